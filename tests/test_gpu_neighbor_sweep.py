"""chb_audit_rows_multi / chb_recruit_rows_multi / clustering.neighbor_sweep: a list of m served from one selection pass.

The calls are DEFINED by the single-m calls: slice j of every output is bit for bit what chb_audit_rows / chb_recruit_rows
returns for m = ms[j].  Every comparison with a single-m call below is np.array_equal (+inf compares equal to +inf; no
output of these calls is ever NaN, which is asserted), no case is left out and no tolerance applies.  One small case is
also held straight against the oracle within QP_TOL, so that the new path does not lean on the single-m kernel alone."""
import functools

import numpy as np
import pytest

from test_gpu_audit import CASES as AUDIT_CASES, case_data as audit_case_data, oracle_rows
from test_gpu_recruit import QP_TOL, check_reduction

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
MS = (5, 1, 16, 3, 8)
N, D, B = 1500, 21, 6
SIZES = (0, 1, 3, 17, 70)   # bins 0 .. 4; bin 5 takes the rest


@functools.lru_cache(maxsize=None)
def sweep_data():
    """(X, labels, Y): N = 1500 rows of D = 21 columns (no multiple of the 8-column chunk), B = 6 bins of 0, 1, 3, 17, 70
    and about 1150 members (an empty bin, fewer members than several list entries, just over one and over several 64-member
    tiles), rows labelled -1 and 99, twins inside a bin and across two bins, and a block of lattice points whose mutual
    distances tie exactly, spread over the sample indices so that the order by index decides among them.
    Y: 70 rows to recruit, new rows (some on the lattice) mixed with exact copies of samples."""
    rng = np.random.default_rng(20261019)
    centres = rng.normal(size=(B, D)) * 0.3
    labels = np.full(N, 5, dtype=np.int64)
    order = rng.permutation(N)
    at = 0
    for b, n in enumerate(SIZES):
        labels[order[at:at + n]] = b
        at += n
    labels[order[at:at + 150]] = -1
    labels[order[at + 150:at + 190]] = 99
    X = centres[np.clip(labels, 0, B - 1)] + rng.normal(size=(N, D)) * 0.2
    # lattice block: {-1, 0, 1}^4 * 0.25 in the first four columns, zero elsewhere: 81 points with exactly representable
    # squared distances, many of them equal; 60 in bin 5, 12 in bin 4, 5 in bin 3, 4 unassigned
    grid = np.stack(np.meshgrid(*([[-0.25, 0.0, 0.25]] * 4), indexing="ij"), axis=-1).reshape(81, 4)
    grid = grid[rng.permutation(81)]
    big, b4, b3, un = (np.flatnonzero(labels == v) for v in (5, 4, 3, -1))
    lat = np.concatenate([rng.choice(big, 60, replace=False), rng.choice(b4, 12, replace=False),
                          rng.choice(b3, 5, replace=False), rng.choice(un, 4, replace=False)])
    X[lat] = 0.0
    X[lat, :4] = grid
    # twins: inside bin 5, inside bin 4, across bins 4 / 5 and 3 / 5, and an unassigned copy of a member of bin 2
    free5 = np.setdiff1d(big, lat)
    free4 = np.setdiff1d(b4, lat)
    a5 = rng.choice(free5, 60, replace=False)
    X[a5[:20]] = X[a5[20:40]]
    X[free4[:4]] = X[free4[4:8]]
    X[free4[8:14]] = X[a5[40:46]]
    X[np.setdiff1d(b3, lat)[:3]] = X[a5[46:49]]
    X[np.setdiff1d(un, lat)[:2]] = X[np.flatnonzero(labels == 2)[0]]
    assert [int(np.count_nonzero(labels == b)) for b in range(5)] == list(SIZES)
    # rows to recruit: 25 new rows of the same clouds, 15 lattice points shifted by half a cell (ties again), 30 copies
    Yn = centres[rng.integers(0, B, 25)] + rng.normal(size=(25, D)) * 0.2
    Yl = np.zeros((15, D))
    Yl[:, :4] = grid[:15] + 0.125
    Y = np.concatenate([Yn, Yl, X[rng.choice(N, 30, replace=False)]])[rng.permutation(70)]
    X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
    for a in (X, labels, Y):
        a.setflags(write=False)
    return X, labels, Y


def same(a, b):
    """bit for bit, as np.array_equal sees it: equal values, +inf included; NaN nowhere"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        assert not np.isnan(a).any() and not np.isnan(b).any()
    assert np.array_equal(a, b)


def check_slices(multi, singles):
    """multi = (bins, dist, mind, margin) of a list call, singles[j] = the same of the single call for its entry j"""
    assert multi[0].shape[0] == len(singles)
    for j, one in enumerate(singles):
        for got, want in zip(multi, one):
            same(got[j], want)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("metric", ["convex", "affine"])
def test_audit_every_row(ctx, metric):
    X, labels, _ = sweep_data()
    ctx.set_samples(X)
    with ctx.using_metric(metric):
        multi = ctx.audit_rows_multi(labels, B, MS)
        singles = [ctx.audit_rows(labels, B, m) for m in MS]
    assert multi[0].shape == (len(MS), N) and multi[1].shape == (len(MS), N, B)
    check_slices(multi, singles)
    # the data does what it was made for: an empty bin, ties decided by index, twins at distance 0
    dist = multi[1]
    assert np.all(np.isinf(dist[:, :, 0])) and np.isfinite(dist[:, :, 2:]).all()
    assert np.count_nonzero(dist[MS.index(1)] == 0.0) > 40
    assert not np.array_equal(dist[MS.index(3)], dist[MS.index(16)])


def test_recruit_new_rows_and_copies(ctx):
    X, labels, Y = sweep_data()
    assert Y.shape == (70, D)
    ctx.set_samples(X)
    multi = ctx.recruit_rows_multi(labels, B, MS, Y)
    singles = [ctx.recruit_rows(labels, B, m, Y) for m in MS]
    check_slices(multi, singles)
    # a copy of a labelled sample has that sample as a candidate: distance 0 at every m
    match = (Y[:, None, :] == X[None, :, :]).all(axis=2)
    assert np.count_nonzero(match.any(axis=1)) >= 30
    of_member = (match & ((labels >= 0) & (labels < B))[None, :]).any(axis=1)
    assert np.count_nonzero(of_member) >= 15 and np.all(multi[2][:, of_member] == 0.0)
    # without the distances
    bins, dist, mind, margin = ctx.recruit_rows_multi(labels, B, MS, Y, want_dist=False)
    assert dist is None
    same(bins, multi[0]); same(mind, multi[2]); same(margin, multi[3])


def test_chunk_edges(ctx):
    X, labels, _ = sweep_data()
    rng = np.random.default_rng(5)
    Q = 1024 + 64 + 7
    rows = rng.integers(0, N, Q).astype(np.int64)
    assert len(np.unique(rows)) < Q
    ctx.set_samples(X)
    before = ctx.counter("recruit_chunk")
    for ms, per_launch in ((tuple(int(m) for m in rng.permutation(16) + 1), 1024), ((7, 2, 11), 5440)):
        multi = ctx.audit_rows_multi(labels, B, ms, rows)
        assert ctx.counter("recruit_multi_rows") == per_launch
        check_slices(multi, [ctx.audit_rows(labels, B, m, rows) for m in ms])
        assert ctx.counter("recruit_multi_rows") == per_launch   # (the single calls leave it alone)
    assert ctx.counter("recruit_chunk") == before == 16384
    # profile: a chunk of 1024 rows and one of 71 for a list of 16; work units = (row, bin, m) triples
    ms = tuple(range(1, 17))
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.audit_rows_multi(labels, B, ms, rows)
    p, single, rm = ctx.profile_get("audit_multi"), ctx.profile_get("audit"), ctx.profile_get("recruit_multi")
    ctx.profile_enable(False)
    assert p["launches"] == 2 and p["work"] == Q * B * 16 and p["ms"] > 0.0
    assert single["launches"] == 0 and rm["launches"] == 0


def test_one_entry_and_reversed_list(ctx):
    X, labels, Y = sweep_data()
    rows = np.arange(0, N, 3, dtype=np.int64)
    ctx.set_samples(X)
    for m in (1, 4, 16):
        check_slices(ctx.audit_rows_multi(labels, B, (m,), rows), [ctx.audit_rows(labels, B, m, rows)])
        check_slices(ctx.recruit_rows_multi(labels, B, [m], Y), [ctx.recruit_rows(labels, B, m, Y)])
    fwd = ctx.audit_rows_multi(labels, B, MS, rows)
    rev = ctx.audit_rows_multi(labels, B, MS[::-1], rows)
    for a, b in zip(fwd, rev):
        same(a, b[::-1])
    fwd = ctx.recruit_rows_multi(labels, B, MS, Y)
    rev = ctx.recruit_rows_multi(labels, B, MS[::-1], Y)
    for a, b in zip(fwd, rev):
        same(a, b[::-1])


def test_against_the_oracle(ctx):
    """Straight against the oracle, not through the single-m kernel: the audit suite's case with a bin of one member, a bin
    of two and a bin of none (N = 400, D = 64, B = 7), every fourth row and all members of the small bins, ms = (1, 4, 16).
    Finite entries within QP_TOL, the +inf pattern exactly, the reduction exactly from the call's own distances."""
    nb = AUDIT_CASES["small_and_empty_bins"]["B"]
    X, labels, _ = audit_case_data("small_and_empty_bins")
    rows = np.union1d(np.arange(0, len(X), 4), np.flatnonzero(labels >= nb - 3)).astype(np.int64)
    ms = (1, 4, 16)
    ctx.set_samples(X)
    bins, dist, mind, margin = ctx.audit_rows_multi(labels, nb, ms, rows)
    for j, m in enumerate(ms):
        want = oracle_rows(X, labels, rows, nb, m)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(dist[j]), fin) and not np.isnan(dist[j]).any()
        assert np.array_equal(dist[j][~fin], want[~fin])
        err = np.abs(dist[j][fin] - want[fin]).max()
        print(f"m = {m}: largest |distance - oracle| = {err:.3e}")
        assert err <= QP_TOL, (m, err)
        check_reduction(bins[j], dist[j], mind[j], margin[j])


def _raw(ctx, labels, nb, ms, nm, rows, Q, bins=True, dist=False, recruit=None, ncol=D):
    """chb_audit_rows_multi, or chb_recruit_rows_multi of the rows `recruit`, through raw ctypes; the outputs are scratch"""
    lib = ctx._lib
    slices = max(min(nm, 16), 1) * max(Q, 1)
    b = np.zeros(slices, dtype=np.int64)
    d = np.zeros(slices * max(min(nb, 8193), 1))
    msa = None if ms is None else np.ascontiguousarray(ms, dtype=np.intc)
    args = [ctx._h, None if labels is None else labels.ctypes.data, nb, None if msa is None else msa.ctypes.data, nm]
    if recruit is None:
        args += [None if rows is None else rows.ctypes.data, Q]
        fn = lib.chb_audit_rows_multi
    else:
        args += [recruit.ctypes.data, Q, ncol]
        fn = lib.chb_recruit_rows_multi
    return fn(*args, b.ctypes.data if bins else None, d.ctypes.data if dist else None, None, None)


def test_abi_refusals():
    from chbin_amd import _lib, synth
    X, labels, Y = sweep_data()
    rows = np.arange(0, N, 11, dtype=np.int64)
    Q = len(rows)
    ms = (5, 2, 9)
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib
        assert _raw(ctx, labels, B, ms, 3, rows, Q) == ESTATE      # no samples
        assert _raw(ctx, labels, B, ms, 3, None, 70, recruit=Y) == ESTATE
        ctx.set_samples(X)
        ref = ctx.audit_rows_multi(labels, B, ms, rows)

        def usable():   # the context still answers, and with the same bits
            for a, b in zip(ctx.audit_rows_multi(labels, B, ms, rows), ref):
                same(a, b)

        for kw in (dict(), dict(recruit=Y)):
            q = 70 if kw else Q
            assert _raw(ctx, labels, B, ms, 3, rows, q, **kw) == 0
            # the list
            assert _raw(ctx, labels, B, None, 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, ms, 0, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, list(range(1, 17)) + [3], 17, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, (5, 2, 5), 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, (5, 0, 2), 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, (5, -3, 2), 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, (5, 17, 2), 3, rows, q, **kw) == EUNSUPPORTED
            assert b"16" in lib.chb_last_error()
            assert _raw(ctx, labels, B, list(range(16, 0, -1)), 16, rows, 3, **kw) == 0
            # the single-m calls' rules
            assert _raw(ctx, labels, 8193, ms, 3, rows, q, **kw) == EUNSUPPORTED
            assert b"8192" in lib.chb_last_error()
            assert _raw(ctx, labels, 0, ms, 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, ms, 3, rows, -1, **kw) == EINVAL
            assert _raw(ctx, None, B, ms, 3, rows, q, **kw) == EINVAL
            assert _raw(ctx, labels, B, ms, 3, rows, q, bins=False, dist=False, **kw) == EINVAL
            assert _raw(ctx, labels, B, ms, 3, rows, q, bins=False, dist=True, **kw) == 0
            usable()
        assert lib.chb_audit_rows_multi(None, labels.ctypes.data, B, np.array(ms, dtype=np.intc).ctypes.data, 3,
                                        rows.ctypes.data, Q, None, None, None, None) == EINVAL
        # NULL row_idx: Q must be N
        assert _raw(ctx, labels, B, ms, 3, None, N) == 0
        assert _raw(ctx, labels, B, ms, 3, None, N - 1) == EINVAL
        assert _raw(ctx, labels, B, ms, 3, None, N + 1) == EINVAL
        # row_idx out of range: refused before anything is enqueued (the outputs stay as they were)
        msa = np.array(ms, dtype=np.intc)
        for bad in (-1, N):
            r = rows.copy()
            r[Q // 2] = bad
            out = np.full(3 * Q, -5, dtype=np.int64)
            rc = lib.chb_audit_rows_multi(ctx._h, labels.ctypes.data, B, msa.ctypes.data, 3, r.ctypes.data, Q,
                                          out.ctypes.data, None, None, None)
            assert rc == EINVAL and np.all(out == -5)
            assert b"row_idx" in lib.chb_last_error()
        # D must be the resident D
        assert _raw(ctx, labels, B, ms, 3, None, 70, recruit=Y, ncol=D - 1) == EINVAL
        assert _raw(ctx, labels, B, ms, 3, None, 70, recruit=Y, ncol=D + 3) == EINVAL
        usable()
        # Q = 0: CHB_OK, nothing is read or written (NULL labels and rows, and with NULL row_idx Q need not be N)
        out = np.full(8, -5, dtype=np.int64)
        dd = np.full(8, -5.0)
        assert lib.chb_audit_rows_multi(ctx._h, None, B, msa.ctypes.data, 3, None, 0, out.ctypes.data, dd.ctypes.data,
                                        dd.ctypes.data, dd.ctypes.data) == 0
        assert lib.chb_recruit_rows_multi(ctx._h, None, B, msa.ctypes.data, 3, None, 0, D, out.ctypes.data, dd.ctypes.data,
                                          dd.ctypes.data, dd.ctypes.data) == 0
        assert np.all(out == -5) and np.all(dd == -5.0)
        usable()

        # ---- an open stepwise fit: refused, and the fit finishes with the labels it would have had
        Xf, initial, _ = synth.make_synthetic(700, 64, 5, seed=3, sigma=6e-3, mix=0.5)
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        K = len(sl)
        flab = np.where(initial >= 0, initial, 0)
        frow = np.arange(0, 700, 9, dtype=np.int64)

        def stepwise(interfere):
            def refused():
                if not interfere:
                    return
                assert _raw(ctx, flab, 5, ms, 3, frow, len(frow)) == ESTATE
                assert _raw(ctx, flab, 5, ms, 3, None, 700, bins=False, dist=True) == ESTATE
                assert _raw(ctx, flab, 5, ms, 3, None, 8, recruit=Xf[:8].copy(), ncol=64) == ESTATE

            ctx.set_samples(Xf)
            ctx.fit_begin(5, initial, 5)
            refused()
            ctx.batch_begin(sl, 0, K)
            refused()
            guess = np.full(K, -1, dtype=np.int64)
            ctx.batch_guess(guess)
            lab1, md1 = np.full(K, -9, dtype=np.int64), np.zeros(K)
            ctx.batch_round(guess, 0, lab1, md1)
            refused()
            ctx.batch_commit(lab1)
            refused()
            # (the labels: a round's min_dist is not promised bit for bit from one fit to the next)
            return lab1.copy(), ctx.fit_labels().copy()

        with_calls, without = stepwise(True), stepwise(False)
        for a, b in zip(with_calls, without):
            same(a, b)
        assert np.all(with_calls[0] >= 0)
        # chb_set_samples ends the stepwise fit
        ctx.set_samples(X)
        usable()
    finally:
        ctx.close()


COUNTERS = ("lookahead_batches", "lookahead_failed", "exchanges", "pack_incremental_batches", "pack_builds", "pool_batches",
            "pool_state", "pool_candidates", "pool_pairs", "fused_enabled", "segment_batches", "batch_size",
            "tile_skip_state", "tile_skipped", "tile_seen", "tile_unloaded", "last_batch_k", "recruit_chunk", "kmer_chunks",
            "prefilter_enabled", "prefilter_overflow", "shortlist_short")


def test_no_trace_left_in_a_fit():
    """set_samples, (a list call,) fit_cluster on a fresh context: labels, sweeps, change counts, chb_fit_stats and the
    counters a fit leaves behind are the same with and without the call; the call itself changes no counter but its own."""
    from chbin_amd import _lib, synth
    n, d, nb, m, its = 2000, 136, 8, 5, 3
    X, initial, _ = synth.make_synthetic(n, d, nb, seed=n + d + nb + m, sigma=6e-3, mix=0.5)
    perms = synth.draw_permutations(initial, its, seed=0)
    Y = X[::40] + 1e-3

    def fit(with_call):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            if with_call:
                before = [ctx.counter(c) for c in COUNTERS]
                stats = ctx.fit_stats()
                assert ctx.counter("recruit_multi_rows") == 0
                bins, _, _, _ = ctx.audit_rows_multi(initial, nb, (3, 15, 5), want_dist=False)
                assert bins.shape == (3, n)
                ctx.recruit_rows_multi(initial, nb, (2, 16), Y)
                assert ctx.counter("recruit_multi_rows") == 8192
                assert [ctx.counter(c) for c in COUNTERS] == before and ctx.fit_stats() == stats
            lab, sweeps, changed = ctx.fit_cluster(nb, initial, perms, m, its)
            return lab, sweeps, changed, [ctx.counter(c) for c in COUNTERS], ctx.fit_stats()
        finally:
            ctx.close()

    a, b = fit(True), fit(False)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a[3] == b[3], (a[3], b[3])
    assert a[4] == b[4]


def test_neighbor_sweep_mirror():
    import chbin_amd
    from chbin_amd import _lib, clustering
    X, labels, _ = sweep_data()
    ms = (1, 3, 5, 10, 15)
    sweep = clustering.neighbor_sweep(X, labels, B)
    assert isinstance(sweep, clustering.NeighborSweep) and tuple(sweep.neighbors) == ms and sweep.distances is None
    audits = [clustering.audit(X, labels, B, num_neighbors=m) for m in ms]
    bins = np.stack([a[0] for a in audits])
    same(sweep.bins, bins)
    same(sweep.min_dist, np.stack([a[1] for a in audits]))
    same(sweep.margin, np.stack([a[2] for a in audits]))
    same(sweep.rows, np.arange(N, dtype=np.int64))
    same(sweep.own, labels)
    inside = (labels >= 0) & (labels < B)
    want_moved = np.array([np.count_nonzero((b != labels) & inside) for b in bins])
    assert np.array_equal(sweep.moved, want_moved) and want_moved.min() > 0
    want_agree = np.array([[np.mean(x == y) for y in bins] for x in bins])
    assert np.array_equal(sweep.agreement, want_agree) and want_agree.min() < 1.0
    want_stable = inside & np.all([(a[0] == labels) & (a[2] > 0.0) for a in audits], axis=0)
    assert np.array_equal(sweep.stable(), want_stable) and want_stable.any() and not want_stable.all()
    # chosen rows, another metric and order, the distances
    rows = np.arange(5, N, 7, dtype=np.int64)
    got = chbin_amd.neighbor_sweep(X, labels, B, neighbors=[16, 2], metric="affine", qp_solver="cvxopt", rows=rows,
                                   return_distances=True)
    for j, m in enumerate((16, 2)):
        ab, am, ag, ad = clustering.audit(X, labels, B, num_neighbors=m, metric="affine", rows=rows, return_distances=True)
        same(got.bins[j], ab); same(got.min_dist[j], am); same(got.margin[j], ag); same(got.distances[j], ad)
    same(got.rows, rows); same(got.own, labels[rows])
    assert _lib.default_context().get_metric() == "convex"
    with pytest.raises(NotImplementedError, match="Unknown solver"):
        clustering.neighbor_sweep(X, labels, B, qp_solver="gurobi")
    with pytest.raises(NotImplementedError, match="Metric"):
        clustering.neighbor_sweep(X, labels, B, metric="euclid")
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep(X, labels, B, neighbors=(3, 3))
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep(X, labels, B, neighbors=(3, 17))
