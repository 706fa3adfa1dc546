"""chb_recruit_rows / Context.recruit_rows / clustering.recruit: hull distances of rows that are NOT samples to every bin of
a frozen labelling, against the oracle.

Oracle for row q (existing oracle functions only): Z = vstack(X, Y), the labels extended by -1 for the rows of Y, and
oracle.sweep(Z, B, labels_ext, [N + q], m, want_all=True) -- sweep copies the labels, so every call sees the frozen state
and the other rows of Y are never members.  Finite entries must agree to QP_TOL = 1e-9 (the project's bound of
test_gpu_bin_distances.py), the +inf pattern exactly.  bin / min_dist / margin are checked exactly against a numpy
strict-'>' scan over the call's own distances, and the bin against the oracle's argmin on every row whose oracle
runner-up gap exceeds 2 * QP_TOL (at most 1 % of a case's rows may be left out by that rule)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QP_TOL = 1e-9

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5

# name: N, D, B, m, Q, generator keywords, metric, transformation
CASES = {
    "base": dict(N=700, D=136, B=6, m=5, Q=300, gen=dict(sigma=6e-3, mix=0.5)),
    # Q no multiple of 64; the 16-lane solver at the reference's default num_neighbors
    "m15": dict(N=700, D=136, B=4, m=15, Q=130, gen=dict(sigma=6e-3, mix=0.5, n_seed=20)),
    # a third of X duplicated, 20 rows of Y copied from X: distance 0 and index-ordered ties at the selection edge
    "m16_dups": dict(N=500, D=64, B=3, m=16, Q=100, gen=dict(sigma=6e-3, mix=0.5, n_seed=20), xform="dups",
                     rseed=16),   # (the seed: by the oracle alone no row then sits on a tie between two bins)
    # wide rows (this path does not depend on the shortlist stage)
    "wide_d300": dict(N=600, D=300, B=4, m=8, Q=100, gen=dict(sigma=6e-3, mix=0.5)),
    "wide_d600": dict(N=400, D=600, B=3, m=5, Q=70, gen=dict(sigma=6e-3, mix=0.5)),
    # one bin of two members, one without any (a +inf column)
    "small_and_empty_bins": dict(N=400, D=64, B=7, m=5, Q=90, gen=dict(sigma=6e-3, mix=0.5, n_seed=8), xform="small_bins"),
    "affine": dict(N=800, D=64, B=6, m=5, Q=120, gen=dict(sigma=8e-3, mix=0.5, n_seed=8), metric="affine"),
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, labels, Y) of a case; deterministic.  labels = the generator's true labels with about 30 % set to -1; Y = rows
    of the same generator that are not in X."""
    from chbin_amd import synth
    c = CASES[name]
    N, D, B, Q = c["N"], c["D"], c["B"], c["Q"]
    Z, _, true = synth.make_synthetic(N + Q, D, B, seed=N + D + B + c["m"], **c["gen"])
    X, Y = Z[:N].copy(), Z[N:].copy()
    rng = np.random.default_rng(c.get("rseed", 7))
    labels = true[:N].copy()
    labels[rng.random(N) < 0.3] = -1
    xf = c.get("xform")
    if xf == "dups":
        X[rng.choice(N, N // 3, replace=False)] = X[rng.choice(N, N // 3, replace=False)]
        Y[rng.choice(Q, 20, replace=False)] = X[rng.choice(N, 20, replace=False)]
    elif xf == "small_bins":
        labels[labels == B - 2] = -1
        labels[labels == B - 1] = -1
        labels[np.flatnonzero(labels == 0)[:2]] = B - 2
    for a in (X, Y, labels):
        a.setflags(write=False)
    return np.ascontiguousarray(X), labels, np.ascontiguousarray(Y)


def oracle_rows(X, labels, Y, B, m, metric="convex", rows=None):
    """[len(rows), B] hull distances of Y[rows] against the frozen labels, by the oracle."""
    from oracle import oracle as O
    N = len(X)
    Z = np.ascontiguousarray(np.vstack([X, Y]))
    lab_ext = np.concatenate([labels, np.full(len(Y), -1, dtype=np.int64)])
    rows = range(len(Y)) if rows is None else rows
    out = np.empty((len(rows), B))
    for k, q in enumerate(rows):
        _, _, alld = O.sweep(Z, B, lab_ext, np.array([N + q], dtype=np.int64), m, want_all=True, metric=metric)
        out[k] = alld[0]
    return out


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    c = CASES[name]
    X, labels, Y = case_data(name)
    d = oracle_rows(X, labels, Y, c["B"], c["m"], c.get("metric", "convex"))
    d.setflags(write=False)
    return d


def strict_scan(dist):
    """(bin, min, margin) of every row by the reference's strict-'>' scan (algorithm.py:57): lowest index among equal
    minima, -1 when every entry is +inf; margin = smallest distance of any other bin minus the minimum, +inf without a
    finite runner-up."""
    Q, B = dist.shape
    bins = np.full(Q, -1, dtype=np.int64)
    mind = np.full(Q, np.inf)
    margin = np.full(Q, np.inf)
    for q in range(Q):
        best, bc = np.inf, -1
        for c in range(B):
            if best > dist[q, c]:
                best, bc = dist[q, c], c
        bins[q], mind[q] = bc, best
        others = np.delete(dist[q], bc) if bc >= 0 else dist[q]
        runner = others.min() if len(others) else np.inf
        margin[q] = np.inf if runner == np.inf else runner - best
    return bins, mind, margin


def check_against_oracle(name, bins, dist, want, cap=0.01):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(dist), fin), name
    assert not np.isnan(dist).any(), name
    assert np.array_equal(dist[~fin], want[~fin]), name   # (+inf, not -inf)
    err = np.abs(dist[fin] - want[fin]).max() if fin.any() else 0.0
    print(f"{name}: largest |distance - oracle| = {err:.3e}")
    assert err <= QP_TOL, (name, err)
    obin, _, omargin = strict_scan(want)
    clear = omargin > 2 * QP_TOL
    left_out = np.count_nonzero(~clear)
    print(f"{name}: {left_out} of {len(bins)} rows within 2 * QP_TOL of a tie, smallest oracle margin {omargin.min():.3e}")
    assert left_out <= cap * len(bins), (name, left_out)
    assert np.array_equal(bins[clear], obin[clear]), name


def check_reduction(bins, dist, mind, margin):
    b, d, g = strict_scan(dist)
    assert np.array_equal(bins, b)
    assert np.array_equal(mind, d)
    assert not np.isnan(margin).any()
    assert np.array_equal(margin, g)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_recruit_matches_oracle(ctx, name):
    c = CASES[name]
    X, labels, Y = case_data(name)
    ctx.set_samples(X)
    with ctx.using_metric(c.get("metric", "convex")):
        bins, dist, mind, margin = ctx.recruit_rows(labels, c["B"], c["m"], Y)
    assert dist.shape == (c["Q"], c["B"])
    check_reduction(bins, dist, mind, margin)
    check_against_oracle(name, bins, dist, case_oracle(name))
    if name == "small_and_empty_bins":
        assert np.all(np.isinf(dist[:, c["B"] - 1])) and np.all(np.isfinite(dist[:, c["B"] - 2]))
    if name == "m16_dups":
        # a row copied from a labelled sample has that sample as a candidate: distance exactly 0
        src = [np.flatnonzero((X == y).all(axis=1)) for y in Y]
        zero = np.array([len(s) > 0 and (labels[s] >= 0).any() for s in src])
        assert zero.sum() > 0 and np.all(mind[zero] == 0.0)


def test_no_labelled_sample_and_single_bin(ctx):
    c = CASES["small_and_empty_bins"]
    X, labels, Y = case_data("small_and_empty_bins")
    ctx.set_samples(X)
    # all labels -1 (and labels outside [0, B), which count as unassigned)
    lab = np.full(len(X), -1, dtype=np.int64)
    lab[::3] = c["B"]
    lab[1::3] = -7
    bins, dist, mind, margin = ctx.recruit_rows(lab, c["B"], c["m"], Y)
    assert np.all(bins == -1)
    assert np.all(dist == np.inf) and np.all(mind == np.inf) and np.all(margin == np.inf)
    # B = 1: every labelled sample in the one bin; no runner-up
    lab1 = np.where(labels >= 0, 0, -1).astype(np.int64)
    bins, dist, mind, margin = ctx.recruit_rows(lab1, 1, c["m"], Y)
    assert np.all(bins == 0) and np.all(np.isfinite(mind)) and np.all(margin == np.inf)
    assert np.array_equal(dist[:, 0], mind)
    rows = list(range(0, len(Y), 9))
    want = oracle_rows(X, lab1, Y, 1, c["m"], rows=rows)
    assert np.abs(dist[rows] - want).max() <= QP_TOL


def test_chunk_edge(ctx):
    """chunk + 1 rows: the second launch of the host loop scores one row.  Every repeat of a row must be bitwise equal to
    its first occurrence, wherever it falls in a chunk."""
    chunk = ctx.counter("recruit_chunk")
    assert chunk > 0
    from chbin_amd import synth
    N, D, B, m, Q0 = 200, 8, 2, 3, 150
    Z, _, true = synth.make_synthetic(N + Q0, D, B, seed=11, sigma=6e-3, mix=0.5)
    X, Y0 = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    labels = true[:N].copy()
    labels[np.random.default_rng(3).random(N) < 0.3] = -1
    Q = chunk + 1
    idx = np.arange(Q) % Q0
    Y = np.ascontiguousarray(Y0[idx])
    ctx.set_samples(X)
    bins, dist, mind, margin = ctx.recruit_rows(labels, B, m, Y)
    want = oracle_rows(X, labels, Y0, B, m)
    check_reduction(bins[:Q0], dist[:Q0], mind[:Q0], margin[:Q0])
    check_against_oracle("chunk_edge", bins[:Q0], dist[:Q0], want)
    assert np.array_equal(dist.view(np.uint64), dist[:Q0][idx].view(np.uint64))
    assert np.array_equal(bins, bins[:Q0][idx])
    assert np.array_equal(mind.view(np.uint64), mind[:Q0][idx].view(np.uint64))
    assert np.array_equal(margin.view(np.uint64), margin[:Q0][idx].view(np.uint64))


def test_one_row_no_row_and_no_distances(ctx):
    c = CASES["base"]
    X, labels, Y = case_data("base")
    want = case_oracle("base")
    ctx.set_samples(X)
    full = ctx.recruit_rows(labels, c["B"], c["m"], Y)
    # Q = 1: the same bits as the row has inside the full call
    one = ctx.recruit_rows(labels, c["B"], c["m"], Y[17:18])
    assert np.abs(one[1][0] - want[17]).max() <= QP_TOL
    for a, b in zip(one, full):
        assert np.array_equal(a, b[17:18])
    # Q = 0
    bins, dist, mind, margin = ctx.recruit_rows(labels, c["B"], c["m"], np.zeros((0, c["D"])))
    assert bins.shape == (0,) and dist.shape == (0, c["B"]) and mind.shape == (0,) and margin.shape == (0,)
    # dist_out = NULL: bins, min and margin only
    bins, dist, mind, margin = ctx.recruit_rows(labels, c["B"], c["m"], Y, want_dist=False)
    assert dist is None
    assert np.array_equal(bins, full[0]) and np.array_equal(mind, full[2]) and np.array_equal(margin, full[3])
    # ... and through the ABI with every optional output NULL but the bins
    lib = ctx._lib
    b2 = np.full(len(Y), -5, dtype=np.int64)
    rc = lib.chb_recruit_rows(ctx._h, labels.ctypes.data, c["B"], c["m"], Y.ctypes.data, len(Y), c["D"], b2.ctypes.data,
                              None, None, None)
    assert rc == 0 and np.array_equal(b2, full[0])
    # profile: one launch, work units = (row, bin) pairs
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.recruit_rows(labels, c["B"], c["m"], Y)
    p = ctx.profile_get("recruit")
    ctx.profile_enable(False)
    assert p["launches"] == 1 and p["work"] == len(Y) * c["B"] and p["ms"] > 0.0


def _raw(ctx, labels, B, m, Y, Q, D, bins=True, dist=False):
    lib = ctx._lib
    b = np.zeros(max(Q, 1), dtype=np.int64)
    d = np.zeros(max(Q, 1) * max(B, 1))
    return lib.chb_recruit_rows(ctx._h, None if labels is None else labels.ctypes.data, B, m,
                                None if Y is None else Y.ctypes.data, Q, D, b.ctypes.data if bins else None,
                                d.ctypes.data if dist else None, None, None)


def test_abi_refusals():
    from chbin_amd import _lib
    c = CASES["base"]
    X, labels, Y = case_data("base")
    N, D, B, m, Q = c["N"], c["D"], c["B"], c["m"], c["Q"]
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib
        # no samples
        assert _raw(ctx, labels, B, m, Y, Q, D) == ESTATE
        ctx.set_samples(X)
        assert _raw(ctx, labels, B, m, Y, Q, D) == 0
        # null arguments
        assert lib.chb_recruit_rows(None, labels.ctypes.data, B, m, Y.ctypes.data, Q, D, None, None, None, None) == EINVAL
        assert _raw(ctx, None, B, m, Y, Q, D) == EINVAL
        assert _raw(ctx, labels, B, m, None, Q, D) == EINVAL
        assert _raw(ctx, labels, B, m, Y, Q, D, bins=False, dist=False) == EINVAL
        assert _raw(ctx, labels, B, m, Y, Q, D, bins=False, dist=True) == 0
        assert _raw(ctx, None, B, m, None, 0, D) == 0   # (Q = 0: nothing is read)
        # ranges
        assert _raw(ctx, labels, B, m, Y, -1, D) == EINVAL
        assert _raw(ctx, labels, 0, m, Y, Q, D) == EINVAL
        assert _raw(ctx, labels, B, 0, Y, Q, D) == EINVAL
        assert _raw(ctx, labels, B, m, Y, Q, D - 1) == EINVAL
        assert _raw(ctx, labels, B, m, Y, Q, D + 1) == EINVAL
        # limits
        assert _raw(ctx, labels, B, 17, Y, Q, D) == EUNSUPPORTED
        assert b"16" in lib.chb_last_error()
        assert _raw(ctx, labels, 8193, m, Y, Q, D) == EUNSUPPORTED
        assert b"8192" in lib.chb_last_error()
        assert _raw(ctx, labels, B, 16, Y, 3, D) == 0

        # ---- an open stepwise fit, an open batch: refused, and the batch's next round gives what it gives without
        # the interruption (a second context runs the same calls undisturbed)
        from chbin_amd import synth
        _, initial, _ = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
        initial = initial[:N].copy()
        move = np.flatnonzero(initial == -1)
        sl = np.random.default_rng(5).permutation(move)[:200].astype(np.int64)
        K = len(sl)
        other = _lib.Context(0)
        try:
            other.set_samples(X)
            out = {}
            host_counters = ("lookahead_batches", "lookahead_failed", "exchanges", "pack_incremental_batches", "pack_builds",
                             "pool_batches", "pool_state", "pool_candidates", "pool_pairs", "segment_batches", "batch_size",
                             "tile_skip_state", "tile_skipped", "tile_seen", "tile_unloaded", "last_batch_k", "fused_enabled",
                             "prefilter_enabled")

            def state(cx):   # every counter the context keeps on the host, and the fit statistics
                return [cx.counter(n) for n in host_counters], cx.fit_stats()

            for who, cx in (("disturbed", ctx), ("plain", other)):
                cx.fit_begin(B, initial, m)
                if who == "disturbed":
                    before = state(cx)
                    assert _raw(cx, labels, B, m, Y, Q, D) == ESTATE
                    assert state(cx) == before   # (a refused call leaves the counters and fit_stats as they were)
                cx.batch_begin(sl, 0, K)
                guess = np.full(K, -1, dtype=np.int64)
                cx.batch_guess(guess)
                lab1, md1 = np.full(K, -9, dtype=np.int64), np.zeros(K)
                cx.batch_round(guess, 0, lab1, md1)
                if who == "disturbed":
                    before = state(cx)
                    assert _raw(cx, labels, B, m, Y, Q, D) == ESTATE
                    assert _raw(cx, labels, B, m, Y, Q, D, bins=False, dist=True) == ESTATE
                    assert state(cx) == before
                lab2, md2 = np.full(K, -9, dtype=np.int64), np.zeros(K)
                cx.batch_round(lab1, 0, lab2, md2)
                cx.batch_commit(lab2)
                out[who] = (guess, lab1, md1, lab2, md2, cx.fit_labels())
            # labels exactly; the winning distances to QP_TOL: two contexts running the same rounds do not reproduce them
            # to the last bit (seen without any recruit call in between: the shortlists are filled by atomics, and the
            # order of a shortlist's candidates decides the order of the hull kernel's sums), and a refused call returns
            # before it touches the device or the context
            d, p = out["disturbed"], out["plain"]
            for k in (0, 1, 3, 5):
                assert np.array_equal(d[k], p[k]), k
            for k in (2, 4):
                print(f"min_dist of round {k // 2}: largest difference between the two contexts {np.abs(d[k] - p[k]).max():.3e}")
                assert np.abs(d[k] - p[k]).max() <= QP_TOL
            # chb_set_samples ends the stepwise fit
            assert _raw(ctx, labels, B, m, Y, Q, D) == ESTATE
            ctx.set_samples(X)
            assert _raw(ctx, labels, B, m, Y, Q, D) == 0
        finally:
            other.close()
    finally:
        ctx.close()


def test_no_trace_left_in_a_fit():
    """fit_cluster, recruit_rows, the same fit again on one context: labels, sweeps and change counts identical, and the
    memos a fit leaves behind for the next (pools, tile skipping, pack builds) as without the call in between."""
    from chbin_amd import _lib, synth
    N, D, B, m, its = 2500, 136, 8, 5, 3
    Z, initial, true = synth.make_synthetic(N + 200, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    initial = initial[:N].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    names = ("pool_state", "tile_skip_state", "pack_builds")

    def two_fits(recruit_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(B, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in names], ctx.fit_stats()))
                if k == 0 and recruit_between:
                    bins, dist, _, _ = ctx.recruit_rows(lab, B, m, Y)
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
    X, labels, Y = case_data("base")
    ctx = _lib.default_context()
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.recruit_rows(labels, c["B"], c["m"], Y)
    got = clustering.recruit(X, labels, Y, c["B"], num_neighbors=c["m"])
    assert isinstance(got, np.ndarray) and np.array_equal(got, bins)
    gb, gd = chbin_amd.recruit(X, labels, Y, c["B"], num_neighbors=c["m"], metric="convex", qp_solver="cvxopt",
                               return_distances=True)
    assert np.array_equal(gb, bins) and np.array_equal(gd, dist)
    with ctx.using_metric("affine"):
        ab, ad, _, _ = ctx.recruit_rows(labels, c["B"], c["m"], Y)
    gb, gd = clustering.recruit(X, labels, Y, c["B"], num_neighbors=c["m"], metric="affine", return_distances=True)
    assert np.array_equal(gb, ab) and np.array_equal(gd, ad)
    assert ctx.get_metric() == "convex"
    with pytest.raises(NotImplementedError, match="Unknown solver"):
        clustering.recruit(X, labels, Y, c["B"], qp_solver="gurobi")
    with pytest.raises(NotImplementedError, match="Metric"):
        clustering.recruit(X, labels, Y, c["B"], metric="euclid")
