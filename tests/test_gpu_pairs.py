"""chb_audit_pairs / chb_recruit_pairs / clustering.cohesion: hull distances of a LIST of (row, bin) pairs.

The calls are defined by the dense ones, so the reference of almost every check is chb_audit_rows / chb_recruit_rows on
the same context, compared BITWISE (uint64 views): a pair's distance must be the dense call's entry whatever tile, chunk
and place in the list it falls into.  The dense calls themselves are checked against the oracle by test_gpu_audit.py /
test_gpu_recruit.py; one test here goes to the oracle directly (finite entries within QP_TOL = 1e-9, the project's bound,
the +inf pattern exactly).  That the work is sparse -- and not a dense call with a gather behind it -- is what the tile
counter and the profile entries show."""
import numpy as np
import pytest

import test_gpu_recruit as R
from test_gpu_audit import CASES, QP_TOL, case_data, case_oracle

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def tiles_of(bins, B):
    """sum over the bins of ceil(pairs of the bin / 64)"""
    return int(((np.bincount(bins, minlength=B) + 63) // 64).sum())


# ---- 1. dense equivalence

@pytest.mark.parametrize("name", list(CASES))
def test_dense_equivalence_bitwise(ctx, name):
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data(name)
    N = len(X)
    ctx.set_samples(X)
    rng = np.random.default_rng(21)
    with ctx.using_metric(c.get("metric", "convex")):
        _, dense, _, _ = ctx.audit_rows(labels, B, m)
        # every pair of the grid, shuffled
        order = rng.permutation(N * B)
        rows, bins = order // B, order % B
        got = ctx.audit_pairs(labels, B, m, rows, bins)
        assert got.shape == (N * B,)
        assert np.array_equal(bits(got), bits(dense[rows, bins]))
        assert ctx.counter("pair_tiles") == B * ((N + 63) // 64)
        # a tenth of them, a fifth of those twice
        sub = rng.choice(N * B, N * B // 10, replace=False)
        sub = np.concatenate([sub, sub[: len(sub) // 5]])[rng.permutation(len(sub) + len(sub) // 5)]
        rows, bins = sub // B, sub % B
        assert len(np.unique(sub)) < len(sub)
        got = ctx.audit_pairs(labels, B, m, rows, bins)
        assert np.array_equal(bits(got), bits(dense[rows, bins]))
        assert ctx.counter("pair_tiles") == tiles_of(bins, B)

        if name == "m16_dups":
            # a twin (another sample with the same coordinates) stays a candidate of its bin: exactly 0, also where that
            # bin is the row's own
            groups = {}
            for i, x in enumerate(X):
                groups.setdefault(x.tobytes(), []).append(i)
            inside = (labels >= 0) & (labels < B)
            pr, pb = [], []
            for i in range(N):
                for b in {int(labels[j]) for j in groups[X[i].tobytes()] if j != i and inside[j]}:
                    pr.append(i)
                    pb.append(b)
            pr, pb = np.array(pr), np.array(pb)
            assert len(pr) > 50 and np.count_nonzero(labels[pr] == pb) > 10
            got = ctx.audit_pairs(labels, B, m, pr, pb)
            assert np.all(got == 0.0)
            # ... and a row without a twin in its own bin is withheld from it: not 0
            alone = np.array([i for i in range(N) if inside[i]
                              and not any(j != i and labels[j] == labels[i] for j in groups[X[i].tobytes()])])
            assert len(alone) > 100
            assert np.all(ctx.audit_pairs(labels, B, m, alone, labels[alone]) > 0.0)
        if name == "small_and_empty_bins":
            one, none = B - 3, B - 1
            lone = np.flatnonzero(labels == one)
            assert len(lone) == 1 and np.count_nonzero(labels == none) == 0
            rows = np.concatenate([np.arange(N), lone, [(lone[0] + 1) % N]])
            bins = np.concatenate([np.full(N, none), [one, one]])
            got = ctx.audit_pairs(labels, B, m, rows, bins)
            assert np.all(got[:N] == np.inf)          # the empty bin
            assert got[N] == np.inf                   # the lone member's own pair
            assert np.isfinite(got[N + 1])            # (any other row sees that member)


# ---- 2. oracle

def test_pairs_match_the_oracle(ctx):
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    rng = np.random.default_rng(22)
    rows = rng.integers(0, len(X), 300)
    bins = rng.integers(0, B, 300)
    ctx.set_samples(X)
    got = ctx.audit_pairs(labels, B, m, rows, bins)
    want = case_oracle("base")[rows, bins]   # (oracle_rows over every row of the case, shared with the audit's tests)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and not np.isnan(got).any()
    assert np.array_equal(got[~fin], want[~fin])
    err = np.abs(got[fin] - want[fin]).max()
    print(f"largest |pair distance - oracle| over {fin.sum()} finite pairs = {err:.3e}")
    assert err <= QP_TOL


# ---- 3. tile and chunk edges

def test_tile_and_chunk_edges(ctx):
    from chbin_amd import synth
    chunk = ctx.counter("recruit_chunk")
    assert chunk == 16384
    N, D, B, m = 600, 136, 6, 5   # the data of the audit's test_chunk_edge
    X, _, true = synth.make_synthetic(N, D, B, seed=11, sigma=6e-3, mix=0.5)
    labels = true.copy()
    labels[np.random.default_rng(3).random(N) < 0.3] = -1
    ctx.set_samples(X)
    _, dense, _, _ = ctx.audit_rows(labels, B, m)
    rng = np.random.default_rng(23)

    # a full tile, a full tile and one pair, one pair, none; two more bins with several tiles / a short one
    per_bin = {0: 64, 1: 65, 2: 1, 3: 0, 4: 130, 5: 7}
    bins = np.concatenate([np.full(n, b) for b, n in per_bin.items()])
    rows = rng.integers(0, N, len(bins))
    sh = rng.permutation(len(bins))
    rows, bins = rows[sh], bins[sh]
    got = ctx.audit_pairs(labels, B, m, rows, bins)
    assert np.array_equal(bits(got), bits(dense[rows, bins]))
    assert ctx.counter("pair_tiles") == 1 + 2 + 1 + 0 + 3 + 1

    # chunk + 70 pairs cycling through the (row, bin) combinations: bin 5's run straddles the chunk boundary
    P = chunk + 70
    p = np.arange(P)
    rows, bins = p % N, (p // 7) % B
    per = np.bincount(bins, minlength=B)
    assert per[:5].sum() < chunk < per.sum() and len(np.unique(rows * B + bins)) < P
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_pairs(labels, B, m, rows, bins)
    prof = ctx.profile_get("audit_pairs")
    ctx.profile_enable(False)
    assert np.array_equal(bits(got), bits(dense[rows, bins]))
    key = rows * B + bins
    _, first = np.unique(key, return_index=True)
    first_of = dict(zip(key[first].tolist(), first.tolist()))
    assert np.array_equal(bits(got), bits(got[[first_of[k] for k in key.tolist()]]))   # every repeat = its first occurrence
    assert ctx.counter("pair_tiles") == tiles_of(bins, B)
    assert prof["launches"] == 2 and prof["work"] == P   # one launch per chunk


# ---- 4. the work is sparse

def test_the_work_is_sparse(ctx):
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    rows = np.flatnonzero((labels >= 0) & (labels < B))
    own = labels[rows]
    P = len(rows)
    ctx.set_samples(X)
    _, dense, _, _ = ctx.audit_rows(labels, B, m)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_pairs(labels, B, m, rows, own)
    prof = {k: ctx.profile_get(k) for k in ("audit_pairs", "recruit_pairs", "audit", "recruit", "audit_multi", "bin_report")}
    ctx.profile_enable(False)
    assert np.array_equal(bits(got), bits(dense[rows, own]))
    want_tiles = sum((np.count_nonzero(own == b) + 63) // 64 for b in range(B))
    assert ctx.counter("pair_tiles") == want_tiles < B * ((len(X) + 63) // 64)
    assert prof["audit_pairs"]["work"] == P and prof["audit_pairs"]["launches"] == 1 and prof["audit_pairs"]["ms"] > 0.0
    for k in ("recruit_pairs", "audit", "recruit", "audit_multi", "bin_report"):   # no dense launch, no row reduction
        assert prof[k]["launches"] == 0 and prof[k]["work"] == 0, k


# ---- 5. recruit pairs

@pytest.mark.parametrize("name", ["base", "wide_d300"])
def test_recruit_pairs(ctx, name):
    c = R.CASES[name]
    B, m, Q = c["B"], c["m"], c["Q"]
    X, labels, Y = R.case_data(name)
    Y = Y.copy()
    src = int(np.flatnonzero(labels >= 0)[5])
    Y[3] = X[src]                                   # a row equal to a labelled sample
    rng = np.random.default_rng(24)
    used = np.arange(0, Q, 2)                       # the odd rows of Y are never referenced, row 3 only below
    P = 2 * Q
    row_of = np.concatenate([rng.choice(used, P), [3, 3]])
    bins = np.concatenate([rng.integers(0, B, P), [labels[src], (labels[src] + 1) % B]])
    assert len(np.unique(row_of)) < len(row_of) and len(np.unique(row_of * B + bins)) < len(row_of)
    ctx.set_samples(X)
    _, dense, _, _ = ctx.recruit_rows(labels, B, m, Y)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.recruit_pairs(labels, B, m, Y, row_of, bins)
    prof = {k: ctx.profile_get(k) for k in ("recruit_pairs", "audit_pairs", "recruit", "audit")}
    ctx.profile_enable(False)
    assert got.shape == (P + 2,)
    assert np.array_equal(bits(got), bits(dense[row_of, bins]))
    assert got[P] == 0.0 and got[P + 1] > 0.0
    assert ctx.counter("pair_tiles") == tiles_of(bins, B)
    assert prof["recruit_pairs"]["launches"] == 1 and prof["recruit_pairs"]["work"] == P + 2
    for k in ("audit_pairs", "recruit", "audit"):
        assert prof[k]["launches"] == 0, k
    # one pair of a one-row Y
    one = ctx.recruit_pairs(labels, B, m, Y[3:4], [0], [labels[src]])
    assert one.shape == (1,) and one[0] == 0.0


def test_recruit_pairs_across_chunks(ctx):
    """More pairs than a chunk holds over 40 rows of Y: a row's bits do not depend on the chunk it is packed into."""
    c = R.CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, Y = R.case_data("base")
    Y = np.ascontiguousarray(Y[:40])
    P = ctx.counter("recruit_chunk") + 70
    p = np.arange(P)
    row_of, bins = p % 40, (p // 3) % B
    ctx.set_samples(X)
    _, dense, _, _ = ctx.recruit_rows(labels, B, m, Y)
    got = ctx.recruit_pairs(labels, B, m, Y, row_of, bins)
    assert np.array_equal(bits(got), bits(dense[row_of, bins]))


# ---- 6. refusals, through the raw ABI

def _audit(ctx, labels, B, m, rows, bins, P, out):
    ptr = lambda a: None if a is None else a.ctypes.data
    return ctx._lib.chb_audit_pairs(ctx._h, ptr(labels), B, m, ptr(rows), ptr(bins), P, ptr(out))


def _recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, P, out):
    ptr = lambda a: None if a is None else a.ctypes.data
    return ctx._lib.chb_recruit_pairs(ctx._h, ptr(labels), B, m, ptr(Y), Q, D, ptr(row_of), ptr(bins), P, ptr(out))


def test_abi_refusals():
    from chbin_amd import _lib, synth
    c = R.CASES["base"]
    X, labels, Y = R.case_data("base")
    N, D, B, m, Q = c["N"], c["D"], c["B"], c["m"], c["Q"]
    rng = np.random.default_rng(25)
    P = 90
    rows, row_of, bins = rng.integers(0, N, P), rng.integers(0, Q, P), rng.integers(0, B, P)
    out = np.full(P, -5.0)
    ctx = _lib.Context(0)
    other = _lib.Context(0)
    try:
        lib = ctx._lib
        # no samples
        assert _audit(ctx, labels, B, m, rows, bins, P, out) == ESTATE
        assert _recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, P, out) == ESTATE
        ctx.set_samples(X)
        ref_a = ctx.audit_pairs(labels, B, m, rows, bins)
        ref_r = ctx.recruit_pairs(labels, B, m, Y, row_of, bins)
        assert np.isfinite(ref_a).all() and np.isfinite(ref_r).all()
        tiles = ctx.counter("pair_tiles")
        assert tiles == tiles_of(bins, B)

        def refused(rc, code, text=None):
            assert rc == code, (rc, code)
            assert np.all(out == -5.0)                     # nothing was written
            assert ctx.counter("pair_tiles") == tiles      # ... or counted
            if text is not None:
                assert text in lib.chb_last_error(), lib.chb_last_error()

        # an entry out of range: refused before anything is enqueued
        for bad in (-1, B):
            b2 = bins.copy()
            b2[P // 2] = bad
            refused(_audit(ctx, labels, B, m, rows, b2, P, out), EINVAL, b"bin_idx")
            refused(_recruit(ctx, labels, B, m, Y, Q, D, row_of, b2, P, out), EINVAL, b"bin_idx")
        for bad in (-1, N):
            r2 = rows.copy()
            r2[P - 1] = bad
            refused(_audit(ctx, labels, B, m, r2, bins, P, out), EINVAL, b"row_idx")
        for bad in (-1, Q):
            r2 = row_of.copy()
            r2[0] = bad
            refused(_recruit(ctx, labels, B, m, Y, Q, D, r2, bins, P, out), EINVAL, b"row_of")
        # null arguments, ranges, D
        refused(_audit(ctx, labels, B, m, rows, bins, P, None), EINVAL)
        refused(_recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, P, None), EINVAL)
        refused(_audit(ctx, None, B, m, rows, bins, P, out), EINVAL)
        refused(_audit(ctx, labels, B, m, None, bins, P, out), EINVAL)
        refused(_audit(ctx, labels, B, m, rows, None, P, out), EINVAL)
        refused(_recruit(ctx, labels, B, m, None, Q, D, row_of, bins, P, out), EINVAL)
        refused(_recruit(ctx, labels, B, m, Y, Q, D, None, bins, P, out), EINVAL)
        refused(lib.chb_audit_pairs(None, labels.ctypes.data, B, m, rows.ctypes.data, bins.ctypes.data, P, out.ctypes.data), EINVAL)
        refused(_audit(ctx, labels, B, m, rows, bins, -1, out), EINVAL)
        refused(_audit(ctx, labels, 0, m, rows, bins, P, out), EINVAL)
        refused(_audit(ctx, labels, B, 0, rows, bins, P, out), EINVAL)
        refused(_recruit(ctx, labels, B, m, Y, Q, D - 1, row_of, bins, P, out), EINVAL)
        refused(_recruit(ctx, labels, B, m, Y, Q, D + 1, row_of, bins, P, out), EINVAL)
        refused(_recruit(ctx, labels, B, m, Y, -1, D, row_of, bins, P, out), EINVAL)
        # limits
        refused(_audit(ctx, labels, B, 17, rows, bins, P, out), EUNSUPPORTED, b"16")
        refused(_recruit(ctx, labels, B, 17, Y, Q, D, row_of, bins, P, out), EUNSUPPORTED, b"16")
        refused(_audit(ctx, labels, 8193, m, rows, bins, P, out), EUNSUPPORTED, b"8192")
        refused(_recruit(ctx, labels, 8193, m, Y, Q, D, row_of, bins, P, out), EUNSUPPORTED, b"8192")
        # P = 0: CHB_OK, nothing is read, written or counted
        refused(_audit(ctx, None, B, m, None, None, 0, None), 0)
        refused(_audit(ctx, labels, B, m, rows, bins, 0, out), 0)
        refused(_recruit(ctx, None, B, m, None, 0, D, None, None, 0, None), 0)
        refused(_recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, 0, out), 0)
        assert ctx.audit_pairs(labels, B, m, [], []).shape == (0,)
        # m = 16 and B = 8192 are served (bins past the labels' largest are empty: +inf)
        o3 = np.full(3, -5.0)
        assert _audit(ctx, labels, B, 16, rows, bins, 3, o3) == 0 and np.isfinite(o3).all()
        big = np.array([B - 1, 8191, B], dtype=np.int64)
        assert _audit(ctx, labels, 8192, m, rows, big, 3, o3) == 0
        assert np.isfinite(o3[0]) and o3[1] == np.inf and o3[2] == np.inf
        # the context still answers, with the same bits
        assert np.array_equal(bits(ctx.audit_pairs(labels, B, m, rows, bins)), bits(ref_a))
        assert np.array_equal(bits(ctx.recruit_pairs(labels, B, m, Y, row_of, bins)), bits(ref_r))
        tiles = ctx.counter("pair_tiles")

        # ---- an open stepwise fit: refused, and the fit completes with the labels it gives without the calls
        _, initial, _ = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
        initial = initial[:N].copy()
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        other.set_samples(X)
        res = {}
        for who, cx in (("disturbed", ctx), ("plain", other)):
            cx.fit_begin(B, initial, m)
            if who == "disturbed":
                refused(_audit(ctx, labels, B, m, rows, bins, P, out), ESTATE)
            cx.batch_begin(sl, 0, len(sl))
            guess = np.full(len(sl), -1, dtype=np.int64)
            cx.batch_guess(guess)
            lab1, md1 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(guess, 0, lab1, md1)
            if who == "disturbed":
                refused(_audit(ctx, labels, B, m, rows, bins, P, out), ESTATE)
                refused(_recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, P, out), ESTATE)
            lab2, md2 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(lab1, 0, lab2, md2)
            cx.batch_commit(lab2)
            res[who] = (lab1, lab2, cx.fit_labels())
        for a, b in zip(res["disturbed"], res["plain"]):
            assert np.array_equal(a, b)
        assert np.all(res["plain"][1] >= 0)
        # chb_set_samples ends the stepwise fit
        refused(_audit(ctx, labels, B, m, rows, bins, P, out), ESTATE)
        ctx.set_samples(X)
        assert np.array_equal(bits(ctx.audit_pairs(labels, B, m, rows, bins)), bits(ref_a))
    finally:
        ctx.close()
        other.close()


# ---- 7. no trace in a fit

COUNTERS = ("lookahead_batches", "lookahead_failed", "exchanges", "pack_incremental_batches", "pack_builds", "pool_batches",
            "pool_state", "pool_candidates", "pool_pairs", "segment_batches", "batch_size", "tile_skip_state", "tile_skipped",
            "tile_seen", "tile_unloaded", "last_batch_k", "fused_enabled", "prefilter_enabled", "recruit_chunk",
            "recruit_multi_rows", "kmer_chunks")


def test_no_trace_left_in_a_fit():
    """fit_cluster, the two pair calls, the same fit again on one context: labels, sweeps and change counts identical, every
    counter but "pair_tiles" and the fit statistics as without the calls in between."""
    from chbin_amd import _lib, synth
    N, D, B, m, its = 2500, 136, 8, 5, 3
    Z, initial, _ = synth.make_synthetic(N + 200, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    initial = initial[:N].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    rng = np.random.default_rng(26)
    row_of, ybins = rng.integers(0, len(Y), 500), rng.integers(0, B, 500)

    def two_fits(pairs_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(B, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in COUNTERS], ctx.fit_stats()))
                if k == 0 and pairs_between:
                    assert ctx.counter("pair_tiles") == 0 and np.all((lab >= 0) & (lab < B))
                    own = ctx.audit_pairs(lab, B, m, np.arange(N), lab)
                    assert np.isfinite(own).all()
                    assert ctx.counter("pair_tiles") == tiles_of(lab, B)
                    assert np.isfinite(ctx.recruit_pairs(lab, B, m, Y, row_of, ybins)).all()
                    assert ctx.counter("pair_tiles") == tiles_of(ybins, B)
                    assert [ctx.counter(n) for n in COUNTERS] == res[0][3]
                    assert ctx.fit_stats() == res[0][4]
                    assert np.array_equal(ctx.fit_labels(), lab)   # (the finished fit's labels are still there)
            return res
        finally:
            ctx.close()

    with_calls, without = two_fits(True), two_fits(False)
    for a, b in ((with_calls[0], with_calls[1]), (with_calls[1], without[1]), (with_calls[0], without[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert with_calls[1][3] == without[1][3], (with_calls[1][3], without[1][3])
    assert with_calls[1][4] == without[1][4]


# ---- 8. cohesion

@pytest.mark.parametrize("name", ["base", "affine", "m15"])
def test_cohesion(name):
    from chbin_amd import _lib, clustering
    import chbin_amd
    c = CASES[name]
    B, m, metric = c["B"], c["m"], c.get("metric", "convex")
    X, labels, _ = case_data(name)
    N = len(X)
    got = clustering.cohesion(X, labels, B, num_neighbors=m, metric=metric)
    dist = clustering.audit(X, labels, B, num_neighbors=m, metric=metric, return_distances=True)[3]
    inside = (labels >= 0) & (labels < B)
    assert got.shape == (N,) and np.array_equal(np.isnan(got), ~inside)
    assert np.array_equal(bits(got[inside]), bits(dist[np.flatnonzero(inside), labels[inside]]))
    if name == "m15":   # the wild labels: B itself, a negative one, one beyond 32 bits
        assert (labels == B).any() and (labels == -7).any() and (labels == 2 ** 40).any() and (labels == -1).any()
    # chosen rows, with a repeat and rows that are not scored; the package-level name
    rows = np.concatenate([np.arange(5, N, 9), [5, 5]])
    sub = chbin_amd.cohesion(X, labels, B, num_neighbors=m, metric=metric, qp_solver="cvxopt", rows=rows)
    assert np.array_equal(bits(sub), bits(got[rows]))
    assert _lib.default_context().get_metric() == "convex"
    # the mirror of the pair call
    pr, pb = rows[inside[rows]], labels[rows[inside[rows]]]
    assert np.array_equal(bits(clustering.audit_pairs(X, labels, pr, pb, B, num_neighbors=m, metric=metric)),
                          bits(got[pr]))


def test_recruit_pairs_mirror():
    from chbin_amd import clustering
    c = R.CASES["affine"]
    B, m = c["B"], c["m"]
    X, labels, Y = R.case_data("affine")
    row_of, bins = np.array([7, 7, 0, 119, 7]), np.array([0, B - 1, 2, 3, 0])
    _, dist = clustering.recruit(X, labels, Y, B, num_neighbors=m, metric="affine", return_distances=True)
    got = clustering.recruit_pairs(X, labels, Y, row_of, bins, B, num_neighbors=m, metric="affine")
    assert np.array_equal(bits(got), bits(dist[row_of, bins]))
