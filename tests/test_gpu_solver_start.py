"""The per-lane Wolfe solver's full-set start (min_norm_point<M> in qp_kernels.hip, m <= 8) and the fused m <= 5 kernel's
candidate ids.

min_norm_point<M> first solves on ALL m vertices and is done when every weight is positive; otherwise it runs Wolfe's minor
cycles down from the full set, and where the full set is affinely dependent (duplicates, collinear vertices, m > D + 1) it
starts from the nearest vertex as before.  (1) drives every one of these routes through chb_hull_distance_points, m = 1 .. 8,
D = 3 and 136, against the oracle's Goldfarb-Idnani and its exhaustive enumerator, with QP_TOL and the scale rule of
test_gpu_parity.py::test_hull_distance_points_vs_oracle_and_enumerator.  That the inputs really have supports of every size
is asserted from the enumerator's weights, without a GPU.  (2) runs small fits through the fused kernel -- D = 3 with m = 5
makes the full set dependent in every pair -- with the trim on and off (off: wide and narrow untrimmed pairs both fetch their
own candidate ids), labels, sweeps and change counts against the oracle's."""
import numpy as np
import pytest

QP_TOL = 1e-9   # (test_gpu_parity.py)

MS = range(1, 9)
DS = (3, 136)
PER_SIZE = {5: 10, 8: 10}   # cases built per support size (the census below asks for ten of each at m = 5 and m = 8)


def _support_case(rng, m, D, k, t):
    """A query whose projection on conv(P) has the k vertices P[:k] as its support (k <= D; k = D + 1: a query inside the
    simplex P[:k]), at distance t * (the cloud's scale) from it: next to a vertex (k = 1), an edge (k = 2), a face."""
    s = 0.1 / np.sqrt(D)
    T = s * rng.standard_normal((k, D))
    w = rng.dirichlet(4.0 * np.ones(k))
    w = (w + 0.1 / k) / 1.1                         # weights bounded away from 0: the support is all of T
    x0 = w @ T
    if k > D:
        n = np.zeros(D)
    else:
        # n: a unit normal of aff(T); the other vertices go on the far side of the plane through x0 across n
        A = T[1:] - T[0]
        n = rng.standard_normal(D)
        if k > 1:
            n -= np.linalg.lstsq(A.T, n, rcond=None)[0] @ A
        n /= np.linalg.norm(n)
    others = []
    for _ in range(m - k):
        r = s * rng.standard_normal(D)
        r -= (r @ n) * n
        others.append(x0 + r - rng.uniform(0.3, 1.5) * 0.1 * n if k <= D else x0 + 3.0 * r / np.linalg.norm(r) * 0.1)
    P = np.vstack([T] + others) if others else T
    P = P[rng.permutation(m)]
    return x0 + t * 0.1 * n, P


def hull_cases(m, D):
    """[(kind, x, P)] for m vertices in D dimensions; deterministic."""
    rng = np.random.default_rng(1000 * m + D)
    s = 0.1 / np.sqrt(D)
    out = []
    for _ in range(4):    # inside the cloud: where D allows it, every vertex is in the support
        P = s * rng.standard_normal((m, D))
        out.append(("inside", rng.dirichlet(3.0 * np.ones(m)) @ P + 0.3 * s * rng.standard_normal(D), P))
    for _ in range(3):    # far away
        P = s * rng.standard_normal((m, D))
        out.append(("far", 8.0 * s * np.ones(D) + s * rng.standard_normal(D), P))
    for k in range(1, min(m, D + 1) + 1):
        # (k = D + 1 with more vertices around: the query lies in several simplices and the enumerator may name a smaller
        #  one, so a few more of these)
        for i in range(PER_SIZE.get(m, 3) + (6 if k > D and m in PER_SIZE else 0)):
            x, P = _support_case(rng, m, D, k, (1e-3, 1.0, 0.05)[i % 3])
            out.append((f"support{k}", x, P))
    if m >= 2:            # duplicated vertices: the full-set solve collapses
        for _ in range(3):
            P = s * rng.standard_normal((m, D))
            P[m - 1] = P[0]
            if m >= 4:
                P[m - 2] = P[1]
            out.append(("duplicates", rng.dirichlet(np.ones(m)) @ P + 0.3 * s * rng.standard_normal(D), P))
        P = np.tile(s * rng.standard_normal(D), (m, 1))
        out.append(("one_point", s * rng.standard_normal(D), P))
    if m >= 3:            # collinear vertices
        for _ in range(3):
            P = s * rng.standard_normal((m, D))
            P[2] = 0.3 * P[0] + 0.7 * P[1]
            if m >= 5:
                P[4] = 1.7 * P[0] - 0.7 * P[1]
            out.append(("collinear", P.mean(0) + 0.5 * s * rng.standard_normal(D), P))
    x = s * rng.standard_normal(D)   # every vertex equal to the query
    out.append(("all_equal_query", x, np.tile(x, (m, 1))))
    return out


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def reference(O):
    """{(m, D): [(kind, x, P, oracle distance, enumerator distance, enumerator weights)]}, computed once."""
    ref = {}
    for m in MS:
        for D in DS:
            rows = []
            for kind, x, P in hull_cases(m, D):
                d_en, a_en = O.enum_hull_distance(x, P, return_alpha=True)
                rows.append((kind, x, P, O.convex_hull_distance(x, P), d_en, a_en))
            ref[(m, D)] = rows
    return ref


@pytest.mark.parametrize("m", [5, 8])
@pytest.mark.parametrize("D", DS)
def test_inputs_have_every_support_size(reference, m, D):
    """The condition on the inputs (no GPU): by the enumerator's weights every support size 1 .. min(m, D + 1) occurs at
    least ten times; the dependent sets (m > D + 1, duplicates, collinear vertices) are there as well."""
    rows = reference[(m, D)]
    sizes = np.array([int(np.count_nonzero(a > 0.0)) for *_, a in rows])
    counts = np.bincount(sizes, minlength=m + 2)
    print(f"\nm={m} D={D}: {len(rows)} cases, support sizes 1.. : {counts[1:min(m, D + 1) + 1].tolist()}")
    for k in range(1, min(m, D + 1) + 1):
        assert counts[k] >= 10, (m, D, k, counts.tolist())
    kinds = {r[0] for r in rows}
    assert {"duplicates", "collinear", "one_point", "all_equal_query", "inside", "far"} <= kinds


@pytest.fixture(scope="module")
def ctx():
    import chbin_amd  # noqa: F401
    from chbin_amd import _lib
    return _lib.default_context()


@pytest.mark.gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("D", DS)
def test_hull_distance_points_every_start(ctx, reference, m, D):
    worst = 0.0
    for kind, x, P, d_or, d_en, _ in reference[(m, D)]:
        d, alpha = ctx.hull_distance_points(x, P, want_alpha=True)
        scale = max(np.linalg.norm(P - x, axis=1).max(), 1e-300)
        assert abs(d - d_or) <= QP_TOL + 1e-7 * scale * (d_or < 1e-6 * scale), (m, D, kind, d, d_or)
        assert abs(d - d_en) <= QP_TOL + 1e-7 * scale * (d_en < 1e-6 * scale), (m, D, kind, d, d_en)
        assert np.all(alpha >= 0) and abs(alpha.sum() - 1) < 1e-12, (m, D, kind, alpha)
        assert abs(np.linalg.norm(alpha @ P - x) - d) <= QP_TOL + 1e-7 * scale * (d < 1e-6 * scale), (m, D, kind)
        worst = max(worst, abs(d - d_en))
    print(f"\nm={m} D={D}: {len(reference[(m, D)])} cases, worst |d - enumerator| {worst:.3g}")


FITS = [(D, m) for D in DS for m in (3, 5)]


@pytest.fixture(scope="module")
def fits(O):
    """{(D, m): (X, initial, perms, oracle labels, sweeps, changes)}: N = 2,000, B = 9, six seeds per bin (so that wide
    shortlists are the rule), three sweeps at the most."""
    from chbin_amd import synth
    out = {}
    for D, m in FITS:
        if D == 3:
            # nine separate clouds in space (the generator's rows of D = 3 lie on a plane, where a contig sits inside the
            # hulls of several bins at once and rounding picks among distances of zero): a contig lies inside the hull of
            # its own bin's neighbours or next to it, and m = 5 > D + 1 vertices are dependent in every pair
            rng = np.random.default_rng(40 + D + m)
            true = rng.integers(0, 9, size=2000)
            centres = np.array([[i % 3, i // 3, 0.0] for i in range(9)]) + 0.2 * rng.standard_normal((9, 3))
            X = np.ascontiguousarray(centres[true] + 0.08 * rng.standard_normal((2000, 3)))
            initial = np.full(2000, -1, dtype=np.int64)
            for c in range(9):
                initial[np.flatnonzero(true == c)[:6]] = c
        else:
            X, initial, _ = synth.make_synthetic(2000, D, 9, seed=40 + D + m, sigma=6e-3, mix=0.5, n_seed=6)
        perms = synth.draw_permutations(initial, 3, seed=0)
        out[(D, m)] = (X, initial, perms) + tuple(O.fit_cluster(X, 9, initial, perms, m, 3))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("trim", ["1", "0"])
@pytest.mark.parametrize("D,m", FITS)
def test_fused_fit_equals_the_oracle(fits, D, m, trim):
    from test_gpu_bin_distances import _ctx_env
    X, initial, perms, want, its_o, ch_o = fits[(D, m)]
    ctx = _ctx_env({"CHB_FUSED_TRIM": trim})
    try:
        ctx.set_samples(X)
        lab, its, ch = ctx.fit_cluster(9, initial, perms, m, 3)
        cnt = {k: int(ctx.counter(k)) for k in ("fused_enabled", "shortlist_short", "fused_trim_pairs")}
    finally:
        ctx.close()
    assert cnt["fused_enabled"] == 1 and cnt["shortlist_short"] == 0, cnt
    print(f"\nD={D} m={m} CHB_FUSED_TRIM={trim}: {its} sweeps, changes {ch.tolist()}, counters {cnt}")
    if trim == "0":
        assert cnt["fused_trim_pairs"] == 0, cnt
    assert its == its_o and np.array_equal(ch, ch_o) and np.array_equal(lab, want), (D, m, trim, its, its_o, ch, ch_o)
