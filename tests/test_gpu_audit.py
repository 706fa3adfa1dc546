"""chb_audit_rows / Context.audit_rows / clustering.audit: leave-one-out hull distances of RESIDENT rows to every bin of a
frozen labelling, against the oracle.

Oracle for sample r (existing oracle functions only): oracle.sweep(X, B, labels, [r], m, want_all=True) -- sweep copies the
labels and takes r out of them for its visit (algorithm.py:50), so every call sees the frozen state with only r withheld.
Finite entries must agree to QP_TOL = 1e-9 (the project's bound of test_gpu_bin_distances.py and test_gpu_recruit.py),
the +inf pattern exactly.  bin / min_dist / margin are checked exactly against a numpy strict-'>' scan over the call's own
distances, and the bin against the oracle's argmin on every row whose oracle runner-up gap exceeds 2 * QP_TOL (at most 1 %
of a case's rows may be left out by that rule; by the oracle alone no row of any case is left out: the smallest oracle
margins are base 4.3e-6, m15 4.1e-5, m16_dups 7.1e-6, small_and_empty_bins 7.9e-6, wide_d300 7.2e-7, affine 2.4e-5)."""
import functools

import numpy as np
import pytest

from test_gpu_recruit import QP_TOL, check_against_oracle, check_reduction, strict_scan

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5

# name: N, D, B, m, generator keywords, metric, transformation of the labels / samples, the rows to score
CASES = {
    # every row (rows=None): Q = 700 is no multiple of 64; labelled and unlabelled rows alike
    "base": dict(N=700, D=136, B=6, m=5, gen=dict(sigma=6e-3, mix=0.5)),
    # the 16-lane solver at the reference's default num_neighbors; 130 chosen indices with repeats, among them labelled,
    # unlabelled and out-of-range-labelled rows
    "m15": dict(N=500, D=136, B=4, m=15, gen=dict(sigma=6e-3, mix=0.5, n_seed=20), xform="wild_labels", rows="chosen"),
    # a third of X duplicated: "withhold the index", not "withhold distance 0"
    "m16_dups": dict(N=500, D=64, B=3, m=16, gen=dict(sigma=6e-3, mix=0.5, n_seed=20), xform="dups"),
    # a bin of one member, a bin of two, a bin of none
    "small_and_empty_bins": dict(N=400, D=64, B=7, m=5, gen=dict(sigma=6e-3, mix=0.5, n_seed=8), xform="small_bins"),
    "wide_d300": dict(N=400, D=300, B=3, m=8, gen=dict(sigma=6e-3, mix=0.5)),
    "affine": dict(N=600, D=64, B=6, m=5, gen=dict(sigma=8e-3, mix=0.5, n_seed=8), metric="affine"),
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, labels, rows) of a case; deterministic.  labels = the generator's true labels with about 30 % set to -1; rows =
    None (all of them) or the chosen sample indices."""
    from chbin_amd import synth
    c = CASES[name]
    N, D, B = c["N"], c["D"], c["B"]
    X, _, true = synth.make_synthetic(N, D, B, seed=N + D + B + c["m"], **c["gen"])
    rng = np.random.default_rng(c.get("rseed", 7))
    labels = true.copy()
    labels[rng.random(N) < 0.3] = -1
    xf = c.get("xform")
    if xf == "dups":
        X[rng.choice(N, N // 3, replace=False)] = X[rng.choice(N, N // 3, replace=False)]
    elif xf == "small_bins":
        for b in (B - 3, B - 2, B - 1):
            labels[labels == b] = -1
        labels[np.flatnonzero(labels == 0)[:2]] = B - 2   # two members
        labels[np.flatnonzero(labels == 1)[:1]] = B - 3   # a single member; bin B - 1 has none
    elif xf == "wild_labels":
        wild = rng.choice(N, 60, replace=False)
        labels[wild[:20]] = B
        labels[wild[20:40]] = -7
        labels[wild[40:]] = 2 ** 40
    rows = None
    if c.get("rows") == "chosen":
        inside = np.flatnonzero((labels >= 0) & (labels < B))
        outside = np.flatnonzero(labels == -1)
        wild = np.flatnonzero((labels < -1) | (labels >= B))
        rows = np.concatenate([rng.choice(inside, 60, replace=False), rng.choice(outside, 30, replace=False),
                               rng.choice(wild, 20, replace=False)])
        rows = np.concatenate([rows, rows[:20]])[rng.permutation(130)].astype(np.int64)   # 130 positions, 20 repeats
        rows.setflags(write=False)
    for a in (X, labels):
        a.setflags(write=False)
    return np.ascontiguousarray(X), labels, rows


def oracle_rows(X, labels, rows, B, m, metric="convex"):
    """[len(rows), B] leave-one-out hull distances of the samples `rows` against the frozen labels, by the oracle."""
    from oracle import oracle as O
    memo = {}
    out = np.empty((len(rows), B))
    for k, r in enumerate(rows):
        r = int(r)
        if r not in memo:
            _, _, alld = O.sweep(X, B, labels, np.array([r], dtype=np.int64), m, want_all=True, metric=metric)
            memo[r] = alld[0]
        out[k] = memo[r]
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    c = CASES[name]
    X, labels, rows = case_data(name)
    d = oracle_rows(X, labels, np.arange(len(X)) if rows is None else rows, c["B"], c["m"], c.get("metric", "convex"))
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_audit_matches_oracle(ctx, name):
    c = CASES[name]
    B = c["B"]
    X, labels, rows = case_data(name)
    ctx.set_samples(X)
    with ctx.using_metric(c.get("metric", "convex")):
        bins, dist, mind, margin = ctx.audit_rows(labels, B, c["m"], rows)
    ids = np.arange(len(X)) if rows is None else rows
    assert dist.shape == (len(ids), B)
    check_reduction(bins, dist, mind, margin)
    check_against_oracle(name, bins, dist, case_oracle(name))
    if name == "m15":
        lab = labels[rows]
        assert ((lab >= 0) & (lab < B)).any() and (lab == -1).any() and ((lab < -1) | (lab >= B)).any()
        assert len(np.unique(rows)) < len(rows)
    if name == "small_and_empty_bins":
        one, two, none = B - 3, B - 2, B - 1
        assert np.count_nonzero(labels == one) == 1 and np.count_nonzero(labels == two) == 2
        lone = labels == one
        assert np.all(np.isinf(dist[lone, one])) and np.all(np.isfinite(dist[~lone, one]))   # its own entry only
        assert np.all(np.isfinite(dist[:, two])) and np.all(np.isinf(dist[:, none]))
    if name == "m16_dups":
        # twins: other samples with the same coordinates
        groups = {}
        for i, x in enumerate(X):
            groups.setdefault(x.tobytes(), []).append(i)
        inside = (labels >= 0) & (labels < B)
        n_zero = n_pos = 0
        for i in range(len(X)):
            twins = [j for j in groups[X[i].tobytes()] if j != i]
            twin_bins = {int(labels[j]) for j in twins if inside[j]}
            for b in twin_bins:   # the twin is a candidate of its bin: exactly 0
                assert dist[i, b] == 0.0
                n_zero += 1
            if inside[i] and not twin_bins:   # only the row itself was at distance 0 in its bin, and it is withheld
                assert dist[i, labels[i]] > 0.0
                n_pos += 1
        assert n_zero > 50 and n_pos > 100


def test_against_the_list_route(ctx):
    """topm_per_bin + hull_distance_batch answer the same question through the list kernels: both are within QP_TOL of the
    oracle, so they agree within twice that."""
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    N = len(X)
    ctx.set_samples(X)
    _, dist, _, _ = ctx.audit_rows(labels, B, m)
    rows = np.arange(N, dtype=np.int64)
    idx, _, _ = ctx.topm_per_bin(labels, B, m, rows)
    want = ctx.hull_distance_batch(np.repeat(rows, B), idx.reshape(N * B, m)).reshape(N, B)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(dist))
    assert np.array_equal(dist[~fin], want[~fin])
    err = np.abs(dist[fin] - want[fin]).max()
    print(f"largest |audit - list route| = {err:.3e}")
    assert err <= 2 * QP_TOL


def test_chunk_edge(ctx):
    """chunk + 70 positions cycling through the samples: the second launch of the host loop scores 70 of them.  Every repeat
    of an index must be bitwise equal to its first occurrence, wherever it falls in a chunk."""
    chunk = ctx.counter("recruit_chunk")
    assert chunk == 16384
    from chbin_amd import synth
    N, D, B, m = 600, 136, 6, 5   # (the base case's row width, bins and neighbours: several k-chunks per tile)
    X, _, true = synth.make_synthetic(N, D, B, seed=11, sigma=6e-3, mix=0.5)
    labels = true.copy()
    labels[np.random.default_rng(3).random(N) < 0.3] = -1
    Q = chunk + 70
    rows = (np.arange(Q) % N).astype(np.int64)
    ctx.set_samples(X)
    bins, dist, mind, margin = ctx.audit_rows(labels, B, m, rows)
    check_reduction(bins[:N], dist[:N], mind[:N], margin[:N])
    edge = np.arange(chunk - 8, chunk + 8)   # the positions either side of the chunk boundary
    check_against_oracle("chunk_edge", bins[edge], dist[edge], oracle_rows(X, labels, rows[edge], B, m))
    assert np.array_equal(dist.view(np.uint64), dist[:N][rows].view(np.uint64))
    assert np.array_equal(bins, bins[:N][rows])
    assert np.array_equal(mind.view(np.uint64), mind[:N][rows].view(np.uint64))
    assert np.array_equal(margin.view(np.uint64), margin[:N][rows].view(np.uint64))
    # rows=None is the same call as rows = 0 .. N-1
    for a, b in zip(ctx.audit_rows(labels, B, m), (bins[:N], dist[:N], mind[:N], margin[:N])):
        assert np.array_equal(a, b)


def fit_data(converging):
    from chbin_amd import synth
    N, D, B, m = 2000, 136, 8, 5
    if converging:   # separated bins: the oracle's fit stops after 2 sweeps
        X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + m)
        its = 6
    else:            # overlapping bins, one sweep only: contigs are still moving when the fit stops
        X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=1.2e-2, mix=0.7)
        its = 1
    return X, initial, synth.draw_permutations(initial, its, seed=0), B, m, its


def test_converged_fit_is_a_fixed_point(ctx):
    X, initial, perms, B, m, max_iter = fit_data(True)
    ctx.set_samples(X)
    lab, iters, changed, fit_min, _ = ctx.fit_cluster_margins(B, initial, perms, m, max_iter, want_min_dist=True)
    assert iters < max_iter and changed[iters - 1] == 0
    bins, _, mind, margin = ctx.audit_rows(lab, B, m, want_dist=False)
    movable = initial == -1
    clear = movable & (margin > 2 * QP_TOL)
    left_out = np.count_nonzero(movable & ~clear)
    print(f"{left_out} of {np.count_nonzero(movable)} movable rows within 2 * QP_TOL of a tie, smallest margin "
          f"{margin[movable].min():.3e}")
    assert left_out <= 0.01 * np.count_nonzero(movable)
    assert np.array_equal(bins[clear], lab[clear])
    # the converged last sweep visited every movable row against the final labels: the fit's own winning distance
    err = np.abs(mind[clear] - fit_min[clear]).max()
    print(f"largest |audit min_dist - fit min_dist| = {err:.3e}")
    assert err <= 2 * QP_TOL
    # the fit never visits the seeds; the audit does
    assert np.all(np.isnan(fit_min[~movable]))
    assert np.all(np.isfinite(mind[~movable])) and np.all(np.isfinite(margin[~movable])) and np.all(bins[~movable] >= 0)


def test_unconverged_fit(ctx):
    X, initial, perms, B, m, max_iter = fit_data(False)
    ctx.set_samples(X)
    lab, iters, changed = ctx.fit_cluster(B, initial, perms, m, max_iter)
    assert iters == max_iter and changed[-1] > 0
    bins, dist, mind, margin = ctx.audit_rows(lab, B, m)
    check_reduction(bins, dist, mind, margin)
    print(f"after {iters} sweep: {np.count_nonzero(bins != lab)} of {len(lab)} rows would choose another bin")
    rows = np.sort(np.random.default_rng(1).choice(len(X), 200, replace=False))
    check_against_oracle("unconverged", bins[rows], dist[rows], oracle_rows(X, lab, rows, B, m))


def _raw(ctx, labels, B, m, rows, Q, bins=True, dist=False, extra=False):
    lib = ctx._lib
    b = np.zeros(max(Q, 1), dtype=np.int64)
    d = np.zeros(max(Q, 1) * max(min(B, 8193), 1))
    e = np.zeros((2, max(Q, 1)))
    return lib.chb_audit_rows(ctx._h, None if labels is None else labels.ctypes.data, B, m,
                              None if rows is None else rows.ctypes.data, Q, b.ctypes.data if bins else None,
                              d.ctypes.data if dist else None, e[0].ctypes.data if extra else None,
                              e[1].ctypes.data if extra else None)


def test_abi_refusals():
    from chbin_amd import _lib, synth
    c = CASES["base"]
    X, labels, _ = case_data("base")
    N, B, m = c["N"], c["B"], c["m"]
    rows = np.arange(0, N, 7, dtype=np.int64)
    Q = len(rows)
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib

        def usable():   # the context still answers, and with the same bits
            got = ctx.audit_rows(labels, B, m, rows)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b)

        # no samples
        assert _raw(ctx, labels, B, m, rows, Q) == ESTATE
        ctx.set_samples(X)
        ref = ctx.audit_rows(labels, B, m, rows)
        assert np.abs(ref[1] - case_oracle("base")[rows]).max() <= QP_TOL
        # row_idx out of range: refused before anything is enqueued (the outputs stay as they were)
        for bad in (-1, N):
            r = rows.copy()
            r[Q // 2] = bad
            out = np.full(Q, -5, dtype=np.int64)
            rc = lib.chb_audit_rows(ctx._h, labels.ctypes.data, B, m, r.ctypes.data, Q, out.ctypes.data, None, None, None)
            assert rc == EINVAL and np.all(out == -5)
            assert b"row_idx" in lib.chb_last_error()
            usable()
        # NULL row_idx: Q must be N
        assert _raw(ctx, labels, B, m, None, N) == 0
        assert _raw(ctx, labels, B, m, None, N - 1) == EINVAL
        assert _raw(ctx, labels, B, m, None, N + 1) == EINVAL
        usable()
        # null context / labels, ranges
        assert lib.chb_audit_rows(None, labels.ctypes.data, B, m, rows.ctypes.data, Q, None, None, None, None) == EINVAL
        assert _raw(ctx, None, B, m, rows, Q) == EINVAL
        assert _raw(ctx, labels, B, m, rows, -1) == EINVAL
        assert _raw(ctx, labels, 0, m, rows, Q) == EINVAL
        assert _raw(ctx, labels, B, 0, rows, Q) == EINVAL
        usable()
        # limits
        assert _raw(ctx, labels, B, 17, rows, Q) == EUNSUPPORTED
        assert b"16" in lib.chb_last_error()
        assert _raw(ctx, labels, 8193, m, rows, Q) == EUNSUPPORTED
        assert b"8192" in lib.chb_last_error()
        assert _raw(ctx, labels, B, 16, rows, 3) == 0
        usable()
        # Q = 0: nothing is read, with NULL row_idx too (the one case in which Q need not be N)
        assert _raw(ctx, None, B, m, rows, 0) == 0
        assert _raw(ctx, None, B, m, None, 0) == 0
        usable()
        # the optional outputs
        assert _raw(ctx, labels, B, m, rows, Q, bins=False, dist=False) == EINVAL
        assert _raw(ctx, labels, B, m, rows, Q, bins=False, dist=False, extra=True) == EINVAL
        b2 = np.full(Q, -5, dtype=np.int64)
        d2 = np.full((Q, B), -5.0)
        assert lib.chb_audit_rows(ctx._h, labels.ctypes.data, B, m, rows.ctypes.data, Q, None, d2.ctypes.data, None, None) == 0
        assert lib.chb_audit_rows(ctx._h, labels.ctypes.data, B, m, rows.ctypes.data, Q, b2.ctypes.data, None, None, None) == 0
        assert np.array_equal(d2, ref[1]) and np.array_equal(b2, ref[0])
        bins, dist, mind, margin = ctx.audit_rows(labels, B, m, rows, want_dist=False)
        assert dist is None
        assert np.array_equal(bins, ref[0]) and np.array_equal(mind, ref[2]) and np.array_equal(margin, ref[3])
        # profile: one launch, work units = (row, bin) pairs; nothing booked under recruit's name
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.audit_rows(labels, B, m, rows)
        p, r = ctx.profile_get("audit"), ctx.profile_get("recruit")
        ctx.profile_enable(False)
        assert p["launches"] == 1 and p["work"] == Q * B and p["ms"] > 0.0 and r["launches"] == 0

        # ---- an open stepwise fit: refused, and the fit stays usable
        X2, initial, _ = synth.make_synthetic(N, c["D"], B, seed=N + c["D"] + B + m, **c["gen"])
        assert np.array_equal(X2, X)
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        K = len(sl)
        ctx.fit_begin(B, initial, m)
        assert _raw(ctx, labels, B, m, rows, Q) == ESTATE
        ctx.batch_begin(sl, 0, K)
        assert _raw(ctx, labels, B, m, rows, Q) == ESTATE
        assert _raw(ctx, labels, B, m, None, N, bins=False, dist=True) == ESTATE
        guess = np.full(K, -1, dtype=np.int64)
        ctx.batch_guess(guess)
        lab1, md1 = np.full(K, -9, dtype=np.int64), np.zeros(K)
        ctx.batch_round(guess, 0, lab1, md1)
        assert _raw(ctx, labels, B, m, rows, Q) == ESTATE
        ctx.batch_commit(lab1)
        assert np.all(lab1 >= 0) and np.array_equal(ctx.fit_labels()[sl], lab1)
        # chb_set_samples ends the stepwise fit
        assert _raw(ctx, labels, B, m, rows, Q) == ESTATE
        ctx.set_samples(X)
        usable()
    finally:
        ctx.close()


def test_no_trace_left_in_a_fit():
    """fit_cluster, audit_rows, the same fit again on one context: labels, sweeps and change counts identical, and the memos
    a fit leaves behind for the next (pools, tile skipping, pack builds) as without the call in between."""
    from chbin_amd import _lib, synth
    N, D, B, m, its = 2500, 136, 8, 5, 3
    X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    perms = synth.draw_permutations(initial, its, seed=0)
    names = ("pool_state", "tile_skip_state", "pack_builds")

    def two_fits(audit_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(B, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in names], ctx.fit_stats()))
                if k == 0 and audit_between:
                    bins, dist, _, _ = ctx.audit_rows(lab, B, m)
                    assert np.isfinite(dist).all() and (bins >= 0).all()
                    assert [ctx.counter(n) for n in names] == res[0][3]
                    assert ctx.fit_stats() == res[0][4]
                    assert np.array_equal(ctx.fit_labels(), lab)   # (the finished fit's labels are still there)
            return res
        finally:
            ctx.close()

    with_call, without = two_fits(True), two_fits(False)
    for a, b in ((with_call[0], with_call[1]), (with_call[1], without[1]), (with_call[0], without[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert with_call[1][3] == without[1][3], (with_call[1][3], without[1][3])
    assert with_call[1][4] == without[1][4]
    assert with_call[0][3] == with_call[1][3], (with_call[0][3], with_call[1][3])


def test_mirror_function():
    from chbin_amd import _lib, clustering
    import chbin_amd
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    rows = np.arange(3, len(X), 5, dtype=np.int64)
    ctx = _lib.default_context()
    ctx.set_samples(X)
    bins, dist, mind, margin = ctx.audit_rows(labels, B, m)
    got = clustering.audit(X, labels, B, num_neighbors=m)
    assert len(got) == 3
    for a, b in zip(got, (bins, mind, margin)):
        assert isinstance(a, np.ndarray) and np.array_equal(a, b)
    got = chbin_amd.audit(X, labels, B, num_neighbors=m, metric="convex", qp_solver="cvxopt", rows=rows,
                          return_distances=True)
    assert len(got) == 4
    for a, b in zip(got, (bins[rows], mind[rows], margin[rows], dist[rows])):
        assert np.array_equal(a, b)
    with ctx.using_metric("affine"):
        ab, ad, am, ag = ctx.audit_rows(labels, B, m, rows)
    got = clustering.audit(X, labels, B, num_neighbors=m, metric="affine", rows=rows, return_distances=True)
    for a, b in zip(got, (ab, am, ag, ad)):
        assert np.array_equal(a, b)
    assert ctx.get_metric() == "convex"
    with pytest.raises(NotImplementedError, match="Unknown solver"):
        clustering.audit(X, labels, B, qp_solver="gurobi")
    with pytest.raises(NotImplementedError, match="Metric"):
        clustering.audit(X, labels, B, metric="euclid")
