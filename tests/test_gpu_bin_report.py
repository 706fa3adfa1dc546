"""chb_bin_report / Context.bin_report / clustering.bin_report: chb_audit_rows' answer reduced on the device per (own bin,
bin) pair.

The expectation of every case is built in numpy from chb_audit_rows' own dist_out / bin_out on the same arguments (that
call is pinned to the oracle by test_gpu_audit.py): confusion, unplaced, dcnt, dmin and n_skipped must be equal exactly
(dmin bit for bit), dsum within relative 1e-12 of math.fsum over the same entries -- n * 2^-53 headroom for the n <= a few
thousand terms of a cell, not a measured number -- and bit-identical between two calls."""
import functools
import math

import numpy as np
import pytest

from test_gpu_audit import CASES, case_data

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
DSUM_RTOL = 1e-12

REPORT_CASES = ["base", "m15", "small_and_empty_bins", "m16_dups", "affine"]


def expected(labels, B, rows, bins, dist):
    """(confusion, unplaced, dcnt, dmin, dsum by fsum, n_skipped) from an audit's bins [Q] and dist [Q, B]."""
    ids = np.arange(len(labels)) if rows is None else rows
    own = labels[ids]
    ok = (own >= 0) & (own < B)
    conf = np.zeros((B, B), dtype=np.int64)
    unplaced = np.zeros(B, dtype=np.int64)
    dcnt = np.zeros((B, B), dtype=np.int64)
    dmin = np.full((B, B), np.inf)
    dsum = np.zeros((B, B))
    for a in range(B):
        sel = ok & (own == a)
        bn, d = bins[sel], dist[sel]
        conf[a] = np.bincount(bn[bn >= 0], minlength=B)
        unplaced[a] = np.count_nonzero(bn < 0)
        fin = np.isfinite(d)
        dcnt[a] = fin.sum(axis=0)
        for b in range(B):
            col = d[fin[:, b], b]
            if len(col):
                dmin[a, b] = col.min()
                dsum[a, b] = math.fsum(col)
    return conf, unplaced, dcnt, dmin, dsum, int(np.count_nonzero(~ok))


def check_report(name, got, want):
    conf, unplaced, dcnt, dmin, dsum, skipped = got
    wconf, wunplaced, wdcnt, wdmin, wdsum, wskipped = want
    assert np.array_equal(conf, wconf), name
    assert np.array_equal(unplaced, wunplaced), name
    assert np.array_equal(dcnt, wdcnt), name
    assert np.array_equal(dmin.view(np.uint64), wdmin.view(np.uint64)), name
    assert skipped == wskipped, name
    assert np.all(dsum[wdcnt == 0] == 0.0) and np.all(np.isinf(dmin[wdcnt == 0])), name
    err = np.abs(dsum - wdsum)
    pos = wdsum > 0.0
    rel = (err[pos] / wdsum[pos]).max() if pos.any() else 0.0
    print(f"{name}: largest relative |dsum - fsum| = {rel:.3e} over {int((wdcnt > 0).sum())} cells, most terms "
          f"{int(wdcnt.max())}")
    assert np.all(err <= DSUM_RTOL * np.abs(wdsum)), name


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", REPORT_CASES)
def test_report_matches_the_audit(ctx, name):
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, rows = case_data(name)
    ctx.set_samples(X)
    with ctx.using_metric(c.get("metric", "convex")):
        bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
        got = ctx.bin_report(labels, B, m, rows)
        again = ctx.bin_report(labels, B, m, rows)
    want = expected(labels, B, rows, bins, dist)
    check_report(name, got, want)
    assert np.array_equal(got[4].view(np.uint64), again[4].view(np.uint64))
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
    assert got[0].sum() + got[1].sum() + got[5] == len(bins)
    if name == "m15":   # chosen rows with repeats and wild labels
        assert got[5] > 0 and len(np.unique(rows)) < len(rows)
        lab = labels[rows]
        assert ((lab < -1) | (lab >= B)).any()
    if name == "small_and_empty_bins":
        none = B - 1
        assert np.all(got[2][:, none] == 0) and np.all(np.isinf(got[3][:, none])) and np.all(got[4][:, none] == 0.0)
        assert np.all(got[2][none] == 0) and got[1][none] == 0   # (no row carries the empty bin's label)
        assert (got[2][:, :none].sum(axis=0) > 0).all()
    if name == "base":   # rows=None is rows = 0 .. N-1
        explicit = ctx.bin_report(labels, B, m, np.arange(len(X), dtype=np.int64))
        for a, b in zip(got, explicit):
            assert np.array_equal(a, b)


def test_unplaced_rows(ctx):
    """A labelling whose only bin has a single member: that row has no other member anywhere, so its scan chooses no bin."""
    X, _, _ = case_data("base")
    B, m = 3, 5
    labels = np.full(len(X), -1, dtype=np.int64)
    labels[17] = 1
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows(labels, B, m)
    got = ctx.bin_report(labels, B, m)
    check_report("unplaced", got, expected(labels, B, None, bins, dist))
    assert got[1].tolist() == [0, 1, 0] and got[0].sum() == 0 and got[2].sum() == 0 and got[5] == len(X) - 1


@functools.lru_cache(maxsize=None)
def boundary_data():
    N, D, B = 16700, 8, 3
    X = np.random.default_rng(16700).standard_normal((N, D))
    labels = (np.arange(N) % B).astype(np.int64)
    return X, labels


def test_chunk_boundary(ctx):
    """16 700 rows, every one labelled i % 3: in label order every label's rows span both 16384-row chunks of the call."""
    assert ctx.counter("recruit_chunk") == 16384
    X, labels = boundary_data()
    N, B, m = len(X), 3, 2
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows(labels, B, m)
    got = ctx.bin_report(labels, B, m)
    check_report("chunk_boundary", got, expected(labels, B, None, bins, dist))
    assert got[5] == 0 and got[2].min() > 5000
    again = ctx.bin_report(labels, B, m)
    explicit = ctx.bin_report(labels, B, m, np.arange(N, dtype=np.int64))
    for other in (again, explicit):
        assert np.array_equal(got[4].view(np.uint64), other[4].view(np.uint64))
        for a, b in zip(got, other):
            assert np.array_equal(a, b)
    # the guaranteed order (include/chbin_hip.h): a label's rows in blocks of 64, each block in order, the block sums in order
    want = np.zeros((B, B))
    for a in range(B):
        d = dist[labels == a]
        for b in range(B):
            total = 0.0
            for r0 in range(0, len(d), 64):
                s = 0.0
                for v in d[r0:r0 + 64, b]:
                    if np.isfinite(v):
                        s = s + float(v)
                total = total + s
            want[a, b] = total
    assert np.array_equal(got[4].view(np.uint64), want.view(np.uint64))


def _raw(ctx, labels, B, m, rows, Q, outs=True):
    """chb_bin_report with small outputs only (unplaced and n_skipped) so that a refused B = 8193 needs no B x B array."""
    lib = ctx._lib
    u = np.full(max(min(B, 8193), 1), -5, dtype=np.int64)
    k = np.full(1, -5, dtype=np.int64)
    rc = lib.chb_bin_report(ctx._h, None if labels is None else labels.ctypes.data, B, m,
                            None if rows is None else rows.ctypes.data, Q, None, u.ctypes.data if outs else None, None,
                            None, None, k.ctypes.data if outs else None)
    return rc, u, int(k[0])


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
            for a, b in zip(ctx.bin_report(labels, B, m, rows), ref):
                assert np.array_equal(a, b)

        # no samples
        assert _raw(ctx, labels, B, m, rows, Q)[0] == ESTATE
        ctx.set_samples(X)
        bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
        ref = ctx.bin_report(labels, B, m, rows)
        check_report("refusals", ref, expected(labels, B, rows, bins, dist))
        # every output NULL
        assert _raw(ctx, labels, B, m, rows, Q, outs=False)[0] == EINVAL
        # row_idx out of range: refused before anything is enqueued (the outputs stay as they were)
        for bad in (-1, N):
            r = rows.copy()
            r[Q // 2] = bad
            rc, u, k = _raw(ctx, labels, B, m, r, Q)
            assert rc == EINVAL and np.all(u == -5) and k == -5
            assert b"row_idx" in lib.chb_last_error()
            usable()
        # NULL row_idx: Q must be N
        assert _raw(ctx, labels, B, m, None, N)[0] == 0
        assert _raw(ctx, labels, B, m, None, N - 1)[0] == EINVAL
        assert _raw(ctx, labels, B, m, None, N + 1)[0] == EINVAL
        # null context / labels, ranges
        assert lib.chb_bin_report(None, labels.ctypes.data, B, m, rows.ctypes.data, Q, None, None, None, None, None, None) == EINVAL
        assert _raw(ctx, None, B, m, rows, Q)[0] == EINVAL
        assert _raw(ctx, labels, B, m, rows, -1)[0] == EINVAL
        assert _raw(ctx, labels, 0, m, rows, Q)[0] == EINVAL
        assert _raw(ctx, labels, B, 0, rows, Q)[0] == EINVAL
        usable()
        # limits
        assert _raw(ctx, labels, B, 17, rows, Q)[0] == EUNSUPPORTED
        assert b"16" in lib.chb_last_error()
        assert _raw(ctx, labels, 8193, m, rows, Q)[0] == EUNSUPPORTED
        assert b"8192" in lib.chb_last_error()
        assert _raw(ctx, labels, B, 16, rows, 3)[0] == 0
        usable()
        # Q = 0 (nothing is read, with NULL row_idx too), and rows none of which has a label in [0, B): zero / +inf tables
        outside = np.flatnonzero(labels == -1)[:40].astype(np.int64)
        for lab_arg, row_arg, q in ((None, rows, 0), (None, None, 0), (labels, outside, len(outside))):
            outs = [np.full((B, B), -5, dtype=np.int64), np.full(B, -5, dtype=np.int64), np.full((B, B), -5, dtype=np.int64),
                    np.full((B, B), -5.0), np.full((B, B), -5.0), np.full(1, -5, dtype=np.int64)]
            rc = lib.chb_bin_report(ctx._h, None if lab_arg is None else lab_arg.ctypes.data, B, m,
                                    None if row_arg is None else row_arg.ctypes.data, q, *[o.ctypes.data for o in outs])
            assert rc == 0
            assert not outs[0].any() and not outs[1].any() and not outs[2].any() and not outs[4].any()
            assert np.all(np.isinf(outs[3])) and np.all(outs[3] > 0) and outs[5][0] == q
        usable()
        # each output alone
        for i in range(5):
            outs = [np.full((B, B), -5, dtype=np.int64), np.full(B, -5, dtype=np.int64), np.full((B, B), -5, dtype=np.int64),
                    np.full((B, B), -5.0), np.full((B, B), -5.0)]
            args = [o.ctypes.data if j == i else None for j, o in enumerate(outs)]
            assert lib.chb_bin_report(ctx._h, labels.ctypes.data, B, m, rows.ctypes.data, Q, *args, None) == 0
            assert np.array_equal(outs[i], ref[i])
        # profile: one launch of the report kernel behind one pair of audit launches, work units = scored (row, bin) pairs
        ctx.profile_enable(True)
        ctx.profile_reset()
        ctx.bin_report(labels, B, m, rows)
        p, a, r = ctx.profile_get("bin_report"), ctx.profile_get("audit"), ctx.profile_get("recruit")
        ctx.profile_enable(False)
        scored = Q - ref[5]
        assert 0 < scored < Q
        assert p["launches"] == 1 and p["work"] == scored * B and p["ms"] > 0.0
        assert a["launches"] == 1 and a["work"] == scored * B and r["launches"] == 0

        # ---- an open stepwise fit: refused, and the fit stays usable
        X2, initial, _ = synth.make_synthetic(N, c["D"], B, seed=N + c["D"] + B + m, **c["gen"])
        assert np.array_equal(X2, X)
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        K = len(sl)
        ctx.fit_begin(B, initial, m)
        assert _raw(ctx, labels, B, m, rows, Q)[0] == ESTATE
        ctx.batch_begin(sl, 0, K)
        assert _raw(ctx, labels, B, m, rows, Q)[0] == ESTATE
        guess = np.full(K, -1, dtype=np.int64)
        ctx.batch_guess(guess)
        lab1, md1 = np.full(K, -9, dtype=np.int64), np.zeros(K)
        ctx.batch_round(guess, 0, lab1, md1)
        assert _raw(ctx, labels, B, m, rows, Q)[0] == ESTATE
        ctx.batch_commit(lab1)
        assert np.all(lab1 >= 0) and np.array_equal(ctx.fit_labels()[sl], lab1)
        # chb_set_samples ends the stepwise fit
        assert _raw(ctx, labels, B, m, rows, Q)[0] == ESTATE
        ctx.set_samples(X)
        usable()
    finally:
        ctx.close()


def test_no_trace_left_and_audit_unchanged():
    """A fit's statistics and counters are the same before and after a bin_report, and audit_rows on the same arguments
    returns what it returned before it."""
    from chbin_amd import _lib, synth
    N, D, B, m, its = 1500, 136, 8, 5, 3
    X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    perms = synth.draw_permutations(initial, its, seed=0)
    names = ("pool_state", "tile_skip_state", "pack_builds", "batch_size", "prefilter_overflow", "lookahead_batches")
    ctx = _lib.Context(0)
    try:
        ctx.set_samples(X)
        lab, _, _ = ctx.fit_cluster(B, initial, perms, m, its)
        before = ([ctx.counter(n) for n in names], ctx.fit_stats())
        audit_before = ctx.audit_rows(lab, B, m)
        rep = ctx.bin_report(lab, B, m)
        check_report("after_a_fit", rep, expected(lab, B, None, audit_before[0], audit_before[1]))
        assert ([ctx.counter(n) for n in names], ctx.fit_stats()) == before
        assert np.array_equal(ctx.fit_labels(), lab)
        for a, b in zip(ctx.audit_rows(lab, B, m), audit_before):
            assert np.array_equal(a, b)
        rows = np.arange(5, N, 3, dtype=np.int64)   # (and an audit that downloads after a call that did not)
        for a, b in zip(ctx.audit_rows(lab, B, m, rows), audit_before):
            assert np.array_equal(a, b[rows])
    finally:
        ctx.close()


def test_mirror_function():
    from chbin_amd import _lib, clustering
    import chbin_amd
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    rows = np.arange(3, len(X), 5, dtype=np.int64)
    ctx = _lib.default_context()
    ctx.set_samples(X)
    want = ctx.bin_report(labels, B, m, rows)
    got = clustering.bin_report(X, labels, B, num_neighbors=m, rows=rows)
    assert isinstance(got, clustering.BinReport)
    for a, b in zip((got.confusion, got.unplaced, got.dcnt, got.dmin, got.dsum, got.n_skipped), want):
        assert np.array_equal(a, b)
    assert np.array_equal(np.isnan(got.mean), got.dcnt == 0)
    assert all(a != b and s >= 0.01 for a, b, s in got.confused_pairs(0.01))
    with ctx.using_metric("affine"):
        want = ctx.bin_report(labels, B, m)
    got = chbin_amd.bin_report(X, labels, B, num_neighbors=m, metric="affine", qp_solver="cvxopt")
    for a, b in zip((got.confusion, got.unplaced, got.dcnt, got.dmin, got.dsum, got.n_skipped), want):
        assert np.array_equal(a, b)
    assert ctx.get_metric() == "convex"
    with pytest.raises(NotImplementedError, match="Unknown solver"):
        clustering.bin_report(X, labels, B, qp_solver="gurobi")
    with pytest.raises(NotImplementedError, match="Metric"):
        clustering.bin_report(X, labels, B, metric="euclid")
