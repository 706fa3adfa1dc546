"""chb_audit_rows_grouped / chb_audit_rows_multi_grouped / chb_audit_pairs_grouped / chb_bin_report_grouped and the `groups`
keyword of the clustering mirror: leave-group-out audit.

The calls are defined by the ungrouped ones (include/chbin_hip.h): for a row of group g the grouped result is bit for bit
what chb_audit_rows returns for that row on labels_g, the labels with every member of g set to -1; for a row without a
group it is what chb_audit_rows returns on the labels themselves.  That per-group route is the yardstick of every test
here (float64 bits, +inf included); tests/row_reference.py is the independent one.  The data set and the numpy statement
of the withheld set live in groups_reference.py (its edges are checked without a device in test_audit_groups_cpu.py)."""
import numpy as np
import pytest

import groups_reference as G
import row_reference as R

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
B = G.B
MS = (1, 3, 5, 16)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    c.set_samples(G.group_data()[0])
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        return b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def assert_same(got, want, what):
    for name, a, b in zip(("bin", "dist", "min", "margin"), got, want):
        assert same_bits(a, b), f"{what}: {name} differs"


_tables, _routes = {}, {}


def grouped_table(ctx, m, metric="convex"):
    """(bin, dist, min, margin) of chb_audit_rows_grouped over all rows; computed once, read-only"""
    if (m, metric) not in _tables:
        _, labels, groups = G.group_data()
        with ctx.using_metric(metric):
            out = ctx.audit_rows_grouped(labels, groups, B, m)
        for a in out:
            a.setflags(write=False)
        _tables[m, metric] = out
    return _tables[m, metric]


def group_route(ctx, m, metric="convex"):
    """The same table by the calls that define it: chb_audit_rows on labels_g for the rows of each group g, on the labels
    themselves for the rows without a group; computed once, read-only"""
    if (m, metric) not in _routes:
        _, labels, groups = G.group_data()
        bins = np.full(G.N, -9, dtype=np.int64)
        dist, mind, margin = np.full((G.N, B), np.nan), np.full(G.N, np.nan), np.full(G.N, np.nan)
        done = np.zeros(G.N, dtype=bool)
        with ctx.using_metric(metric):
            lone = np.flatnonzero(groups < 0)
            jobs = [(lone, labels)]
            for g in np.unique(groups[groups >= 0]):
                rows = np.flatnonzero(groups == g)
                assert np.array_equal(G.withheld(groups, rows[0]), rows)
                jobs.append((rows, G.labels_without(labels, groups, rows[0])))
            for rows, lab in jobs:
                b, d, mn, mg = ctx.audit_rows(lab, B, m, rows.astype(np.int64))
                bins[rows], dist[rows], mind[rows], margin[rows] = b, d, mn, mg
                done[rows] = True
        assert done.all()
        out = (bins, dist, mind, margin)
        for a in out:
            a.setflags(write=False)
        _routes[m, metric] = out
    return _routes[m, metric]


# ---- 1. the defining identity
@pytest.mark.parametrize("m,metric", [(m, "convex") for m in MS] + [(5, "affine")])
def test_defining_identity(ctx, m, metric):
    X, labels, groups = G.group_data()
    got, want = grouped_table(ctx, m, metric), group_route(ctx, m, metric)
    assert_same(got, want, f"m={m} {metric}")
    bins, dist, _, _ = got
    # the data set's edges did occur
    every = groups == G.ALL_OF_BIN
    assert np.all(np.isinf(dist[every, G.SMALL_BIN])) and np.all(np.isfinite(dist[~every, G.SMALL_BIN]))
    assert np.all(np.isfinite(dist[:, :3]))
    tw = np.flatnonzero((groups == G.TWINS) & (labels == 0))
    outside = [r for r in np.flatnonzero((X == X[tw[0]]).all(axis=1)) if groups[r] != G.TWINS]
    assert len(tw) == 2 and len(outside) == 1
    # the twin outside the group stays a candidate of bin 0, at distance 0 (exactly 0 where it is the only vertex)
    assert np.all(dist[tw, 0] < 1e-9) and np.all(dist[outside, 0] < 1e-9)
    if m == 1:
        assert np.all(dist[tw, 0] == 0.0) and np.all(dist[outside, 0] == 0.0)
    if metric == "convex" and m == 5:
        plain = ctx.audit_rows(labels, B, m)
        changed = np.flatnonzero((plain[1] != dist).any(axis=1))
        sized = np.array([np.count_nonzero(groups == groups[r]) if groups[r] >= 0 else 1 for r in range(G.N)])
        print(f"{len(changed)} rows differ from the leave-one-out audit")
        assert np.all(sized[changed] > 1) and len(changed) > 30   # only rows with siblings can differ, and many do
        assert same_bits(plain[1][sized == 1], dist[sized == 1])


# ---- 2. no groups is the old call
def test_no_groups_is_the_old_call(ctx):
    _, labels, _ = G.group_data()
    for m in (5, 16):
        want = ctx.audit_rows(labels, B, m)
        assert_same(ctx.audit_rows_grouped(labels, np.full(G.N, -1, dtype=np.int64), B, m), want, "all -1")
        assert_same(ctx.audit_rows_grouped(labels, np.arange(G.N, dtype=np.int64), B, m), want, "all distinct")
        assert_same(ctx.audit_rows_grouped(labels, -1 - (np.arange(G.N, dtype=np.int64) % 2), B, m), want, "two negative values")


# ---- 3. the independent yardstick
@pytest.mark.parametrize("m", [5, 12])
def test_against_the_row_reference(ctx, m):
    X, labels, groups = G.group_data()
    rng = np.random.default_rng(48)
    special = np.concatenate([rng.choice(np.flatnonzero(groups == g), n, replace=False)
                              for g, n in ((G.BIG, 10), (G.ALL_OF_BIN, 4), (G.STARVER, 3), (G.TWINS, 3))])
    pool = np.setdiff1d(np.arange(G.N), special)
    rows = np.concatenate([special, rng.choice(pool[groups[pool] >= 0], 16, replace=False),
                           rng.choice(pool[groups[pool] < 0], 12, replace=False)])
    assert len(rows) == 48 and len(np.unique(rows)) == 48
    refs = [R.reference_rows(X, G.labels_without(labels, groups, int(r)), B, m, rows=[int(r)]) for r in rows]
    ref = R.RowReference(np.vstack([f.dist for f in refs]), np.vstack([f.scale for f in refs]), None)
    bins, dist, _, _ = ctx.audit_rows_grouped(labels, groups, B, m, rows.astype(np.int64))
    fin = np.isfinite(ref.dist)
    assert np.array_equal(fin, np.isfinite(dist)) and np.all(dist[~fin] == np.inf)
    err, bnd = np.abs(dist[fin] - ref.dist[fin]), R.bound(ref)[fin]
    print(f"m={m}: largest |grouped - reference| / bound = {(err[bnd > 0] / bnd[bnd > 0]).max():.3e}, "
          f"{np.count_nonzero(~fin)} +inf")
    assert np.all(err <= bnd)
    want, clear = R.clear_rows(ref)
    print(f"m={m}: {np.count_nonzero(clear)} of 48 rows clear")
    assert np.array_equal(bins[clear], want[clear])


# ---- 4. row list and chunk edge
def test_row_list_and_chunk_edge(ctx):
    _, labels, groups = G.group_data()
    m = 5
    chunk = ctx.counter("recruit_chunk")
    assert chunk == 16384
    Q = chunk + 70
    rows = np.random.default_rng(4).integers(0, G.N, Q).astype(np.int64)   # repeats, out of order
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        got = ctx.audit_rows_grouped(labels, groups, B, m, rows)
        p_grouped = ctx.profile_get("audit")
        ctx.profile_reset()
        ctx.audit_rows(labels, B, m, rows)
        p_plain = ctx.profile_get("audit")
    finally:
        ctx.profile_enable(False)
    assert_same(got, [a[rows] for a in grouped_table(ctx, m)], "row list")
    # the kernel did the withholding: as many launches as the ungrouped call, one per chunk
    assert p_grouped["launches"] == p_plain["launches"] == 2
    assert p_grouped["work"] == p_plain["work"] == Q * B
    assert ctx.counter("recruit_chunk") == chunk


# ---- 5. pairs
def test_pairs(ctx):
    _, labels, groups = G.group_data()
    m = 5
    rng = np.random.default_rng(5)
    big = np.flatnonzero(groups == G.BIG)
    every = np.flatnonzero(groups == G.ALL_OF_BIN)   # (8 rows: +inf for bin 3)
    rows = np.concatenate([big, big, every, rng.integers(0, G.N, 130), rng.integers(0, G.N, 22)])
    bins = np.concatenate([np.zeros(70), np.ones(70), np.full(8, G.SMALL_BIN), rng.integers(0, B, 130), np.full(22, G.SMALL_BIN)])
    rows, bins = np.concatenate([rows, rows[:20]]), np.concatenate([bins, bins[:20]])   # repeats
    order = rng.permutation(len(rows))
    rows, bins = rows[order].astype(np.int64), bins[order].astype(np.int64)
    got = ctx.audit_pairs_grouped(labels, groups, B, m, rows, bins)
    tiles = ctx.counter("pair_tiles")
    assert same_bits(got, grouped_table(ctx, m)[1][rows, bins])
    assert len(rows) == 320 and np.count_nonzero(np.isinf(got)) >= 8
    ctx.audit_pairs(labels, B, m, rows, bins)
    assert tiles == ctx.counter("pair_tiles") > B
    assert same_bits(ctx.audit_pairs(labels, B, m, rows, bins, groups=groups), got)


# ---- 6. a list of m
def test_list_of_m(ctx):
    _, labels, groups = G.group_data()
    ms = (5, 1, 16, 3)
    got = ctx.audit_rows_multi_grouped(labels, groups, B, ms)
    for j, m in enumerate(ms):
        assert_same([a[j] for a in got], grouped_table(ctx, m), f"slice {j} (m={m})")
    rows = np.arange(G.N - 1, -1, -3, dtype=np.int64)
    got = ctx.audit_rows_multi_grouped(labels, groups, B, ms, rows)
    for j, m in enumerate(ms):
        assert_same([a[j] for a in got], [a[rows] for a in grouped_table(ctx, m)], f"rows, slice {j} (m={m})")
    assert ctx.counter("recruit_multi_rows") == 16384 // 4


# ---- 7. bin report
def test_bin_report(ctx):
    _, labels, groups = G.group_data()
    m = 5
    bins, dist, _, _ = grouped_table(ctx, m)
    conf, unplaced, dcnt, dmin, dsum, skipped = ctx.bin_report_grouped(labels, groups, B, m)
    own = labels
    ok = (own >= 0) & (own < B)
    assert skipped == np.count_nonzero(~ok) > 30
    wconf, wunp, wcnt = np.zeros((B, B), dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros((B, B), dtype=np.int64)
    wmin, wsum = np.full((B, B), np.inf), np.zeros((B, B))
    for a in range(B):
        bn, d = bins[ok & (own == a)], dist[ok & (own == a)]
        wconf[a] = np.bincount(bn[bn >= 0], minlength=B)
        wunp[a] = np.count_nonzero(bn < 0)
        fin = np.isfinite(d)
        wcnt[a] = fin.sum(axis=0)
        for b in range(B):
            if fin[:, b].any():
                wmin[a, b] = d[fin[:, b], b].min()
            # the guaranteed order of chb_bin_report: the label's rows in blocks of 64, each block in order, the block
            # sums in order
            total = 0.0
            for r0 in range(0, len(d), 64):
                s = 0.0
                for v in d[r0:r0 + 64, b]:
                    if np.isfinite(v):
                        s = s + float(v)
                total = total + s
            wsum[a, b] = total
    assert np.array_equal(conf, wconf) and np.array_equal(unplaced, wunp) and np.array_equal(dcnt, wcnt)
    assert same_bits(dmin, wmin) and same_bits(dsum, wsum)
    # bin 3's rows are all in one group: none of them has a distance to its own bin
    assert dcnt[G.SMALL_BIN, G.SMALL_BIN] == 0 and conf[G.SMALL_BIN, G.SMALL_BIN] == 0 and np.isinf(dmin[G.SMALL_BIN, G.SMALL_BIN])
    plain = ctx.bin_report(labels, B, m)
    assert plain[2][G.SMALL_BIN, G.SMALL_BIN] == 6
    # a row list with repeats
    rows = np.random.default_rng(7).integers(0, G.N, 300).astype(np.int64)
    got = ctx.bin_report(labels, B, m, rows, groups=groups)
    sel = rows[ok[rows]]
    assert got[5] == len(rows) - len(sel)
    for a in range(B):
        s = sel[labels[sel] == a]
        assert np.array_equal(got[0][a], np.bincount(bins[s][bins[s] >= 0], minlength=B))
        assert np.array_equal(got[2][a], np.isfinite(dist[s]).sum(axis=0))


# ---- 8. refusals leave the outputs untouched
def _raw(lib, h, name, labels, groups, m, rows, Q, nb=B, bins_for_pairs=None):
    """One grouped entry point through raw ctypes with sentinel-filled outputs: (rc, outputs untouched)"""
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    bout = np.full(max(Q, 1) * 4, -5, dtype=np.int64)
    dout = np.full(max(Q, 1) * 4 * min(max(nb, 1), 8), -5.0)
    small = [np.full(min(max(nb, 1), 8) ** 2, -5, dtype=np.int64) for _ in range(3)]
    fl = [np.full(min(max(nb, 1), 8) ** 2, -5.0) for _ in range(2)]
    k = np.full(1, -5, dtype=np.int64)
    if name == "rows":
        rc = lib.chb_audit_rows_grouped(h, p(labels), p(groups), nb, m, p(rows), Q, p(bout), None, None, None)
    elif name == "multi":
        ms = np.array([m, 2], dtype=np.intc)
        rc = lib.chb_audit_rows_multi_grouped(h, p(labels), p(groups), nb, p(ms), 2, p(rows), Q, p(bout), None, None, None)
    elif name == "pairs":
        rc = lib.chb_audit_pairs_grouped(h, p(labels), p(groups), nb, m, p(rows), p(bins_for_pairs), Q, p(dout))
    else:
        # (B x B tables: only the small outputs are handed over, so a refused B = 8193 needs no B x B array)
        rc = lib.chb_bin_report_grouped(h, p(labels), p(groups), nb, m, p(rows), Q, None, p(small[1]) if nb <= 8 else None,
                                        None, None, None, p(k))
    clean = np.all(bout == -5) and np.all(dout == -5.0) and all(np.all(a == -5) for a in small + fl) and k[0] == -5
    return rc, clean


def test_refusals_leave_outputs_untouched():
    from chbin_amd import _lib, synth
    X, labels, groups = G.group_data()
    labels, groups = np.ascontiguousarray(labels), np.ascontiguousarray(groups)
    m = 5
    rows = np.arange(0, G.N, 7, dtype=np.int64)
    Q = len(rows)
    pbins = (np.arange(Q) % B).astype(np.int64)
    names = ("rows", "multi", "pairs", "report")
    ctx = _lib.Context(0)
    try:
        lib, h = ctx._lib, ctx._h

        def call(name, labels=labels, groups=groups, m=m, rows=rows, Q=Q, nb=B):
            return _raw(lib, h, name, labels, groups, m, rows, Q, nb, pbins)

        # no resident samples
        for name in names:
            assert call(name) == (ESTATE, True), name
        ctx.set_samples(X)
        ref = ctx.audit_rows_grouped(labels, groups, B, m, rows)
        for name in names:
            # groups == NULL: the ungrouped call is the one to use
            assert call(name, groups=None) == (EINVAL, True), name
            assert b"groups" in lib.chb_last_error()
            assert call(name, groups=None, Q=0) == (EINVAL, True), name
            # limits
            assert call(name, m=17) == (EUNSUPPORTED, True), name
            assert b"16" in lib.chb_last_error()
            assert call(name, nb=8193) == (EUNSUPPORTED, True), name
            assert b"8192" in lib.chb_last_error()
            # a row_idx entry equal to N (and a negative one)
            for bad in (G.N, -1):
                r = rows.copy()
                r[Q // 2] = bad
                assert call(name, rows=r) == (EINVAL, True), name
                assert b"row_idx" in lib.chb_last_error()
            # Q = 0 / P = 0 is a no-op
            rc, clean = call(name, Q=0)
            assert rc == 0 and (clean or name == "report"), name   # (the report of no rows: zero tables, n_skipped = 0)
        # row_idx == NULL means all rows, and Q must then be N
        assert call("rows", rows=None, Q=G.N)[0] == 0
        assert call("rows", rows=None, Q=G.N - 1) == (EINVAL, True)
        assert_same(ctx.audit_rows_grouped(labels, groups, B, m, rows), ref, "after the refusals")

        # ---- an open stepwise fit: refused, and the fit finishes with the labels it gives without the interruption
        Xf, initial, _ = synth.make_synthetic(G.N, G.D, B, seed=G.N + G.D + B, sigma=6e-3, mix=0.5)
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        K = len(sl)

        def one_batch(c, interrupt):
            def refused():
                for name in names if interrupt else ():
                    assert _raw(c._lib, c._h, name, labels, groups, m, rows, Q, B, pbins) == (ESTATE, True), name

            c.set_samples(Xf)
            c.fit_begin(B, initial, m)
            refused()
            c.batch_begin(sl, 0, K)
            refused()
            guess = np.full(K, -1, dtype=np.int64)
            c.batch_guess(guess)
            lab1, md1 = np.full(K, -9, dtype=np.int64), np.zeros(K)
            c.batch_round(guess, 0, lab1, md1)
            refused()
            c.batch_commit(lab1)
            return lab1, md1, c.fit_labels()

        runs = []
        for interrupt in (True, False):   # the same steps on two contexts of their own, with and without the refused calls
            fresh = _lib.Context(0)
            try:
                runs.append(one_batch(fresh, interrupt))
            finally:
                fresh.close()
        with_calls, without = runs
        assert np.all(with_calls[0] >= 0)
        # the labels.  The round's min_dist is not compared bit for bit: two untouched contexts running these steps give it
        # equal only to about 1e-17 (seen: 52 of 200 entries differ by at most 1.04e-17), with or without a refused call in
        # between; each run is within the project's QP_TOL = 1e-9 of the oracle (test_gpu_stepwise.py), so within twice that
        assert np.array_equal(with_calls[0], without[0]) and np.array_equal(with_calls[2], without[2])
        assert np.abs(with_calls[1] - without[1]).max() <= 2e-9
        again = one_batch(ctx, True)   # ... and on the context of the refusals above
        assert np.array_equal(again[0], without[0]) and np.array_equal(again[2], without[2])
        # chb_set_samples ends the stepwise fit
        ctx.set_samples(X)
        assert_same(ctx.audit_rows_grouped(labels, groups, B, m, rows), ref, "after the stepwise fit")
    finally:
        ctx.close()


# ---- 9. no trace
def test_no_trace():
    from chbin_amd import _lib, synth
    _, labels, groups = G.group_data()
    m, its = 5, 3
    X, initial, _ = synth.make_synthetic(G.N, G.D, B, seed=G.N + G.D + B, sigma=6e-3, mix=0.5)
    perms = synth.draw_permutations(initial, its, seed=0)
    rows = np.arange(1, G.N, 3, dtype=np.int64)

    def run(grouped_first):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            if grouped_first:
                ctx.audit_rows_grouped(labels, groups, B, m)
                ctx.audit_pairs_grouped(labels, groups, B, m, rows, rows % B)
                ctx.bin_report_grouped(labels, groups, B, m)
            fit = ctx.fit_cluster(B, initial, perms, m, its)
            stats = ctx.fit_stats()
            plain = ctx.audit_rows(labels, B, m, rows) + (ctx.audit_pairs(labels, B, m, rows, rows % B),)
            report = ctx.bin_report(labels, B, m)
            return fit, stats, plain, report
        finally:
            ctx.close()

    (fit_a, stats_a, plain_a, rep_a), (fit_b, stats_b, plain_b, rep_b) = run(True), run(False)
    assert np.array_equal(fit_a[0], fit_b[0]) and fit_a[1] == fit_b[1] and np.array_equal(fit_a[2], fit_b[2])
    assert stats_a == stats_b
    for a, b in zip(plain_a + rep_a[:5], plain_b + rep_b[:5]):
        assert same_bits(a, b)
    assert rep_a[5] == rep_b[5]


# ---- 10. the Python layer
def test_python_layer(ctx):
    import chbin_amd
    from chbin_amd import _lib, clustering
    X, labels, groups = G.group_data()
    m = 5
    # one name per sample: the members of a group share one, a sample without a group has its own
    names = [f"parent_{g}" if g >= 0 else f"whole_{i}" for i, g in enumerate(groups.tolist())]
    pg = clustering.parent_groups(names)
    assert pg.dtype == np.int64 and pg.min() == 0
    bins, dist, mind, margin = grouped_table(ctx, m)
    got = clustering.audit(X, labels, B, num_neighbors=m, return_distances=True, groups=pg)
    assert_same((got[0], got[3], got[1], got[2]), (bins, dist, mind, margin), "audit(groups=parent_groups)")
    rows = np.arange(3, G.N, 5, dtype=np.int64)
    got = chbin_amd.audit(X, labels, B, num_neighbors=m, rows=rows, groups=groups)
    assert_same((got[0], dist[rows], got[1], got[2]), (bins[rows], dist[rows], mind[rows], margin[rows]), "audit(rows, groups)")
    # cohesion: the row's own bin, NaN without a label
    ok = (labels >= 0) & (labels < B)
    want = np.full(G.N, np.nan)
    want[ok] = dist[ok, labels[ok]]
    got = clustering.cohesion(X, labels, B, num_neighbors=m, groups=pg)
    assert same_bits(got[ok], want[ok]) and np.all(np.isnan(got[~ok]))
    assert np.all(np.isinf(got[labels == G.SMALL_BIN]))   # bin 3 without the row's own parent is empty
    assert np.all(np.isfinite(clustering.cohesion(X, labels, B, num_neighbors=m)[labels == G.SMALL_BIN]))
    assert same_bits(clustering.cohesion(X, labels, B, num_neighbors=m, rows=rows, groups=groups)[ok[rows]], want[rows][ok[rows]])
    # the other three
    pairs_b = (rows % B).astype(np.int64)
    assert same_bits(clustering.audit_pairs(X, labels, rows, pairs_b, B, num_neighbors=m, groups=pg), dist[rows, pairs_b])
    sweep = clustering.neighbor_sweep(X, labels, B, neighbors=(5, 3), groups=pg, return_distances=True)
    assert_same((sweep.bins[0], sweep.distances[0], sweep.min_dist[0], sweep.margin[0]), (bins, dist, mind, margin), "sweep")
    assert_same((sweep.bins[1], sweep.distances[1], sweep.min_dist[1], sweep.margin[1]), grouped_table(ctx, 3), "sweep, m=3")
    rep = clustering.bin_report(X, labels, B, num_neighbors=m, groups=pg)
    assert rep.dcnt[G.SMALL_BIN, G.SMALL_BIN] == 0 and rep.n_skipped == np.count_nonzero(~ok)
    assert np.array_equal(rep.confusion, ctx.bin_report_grouped(labels, groups, B, m)[0])
    # groups=None takes today's route
    assert_same(clustering.audit(X, labels, B, num_neighbors=m, groups=None)[:1], ctx.audit_rows(labels, B, m)[:1], "None")
    # rows that are not samples have no siblings: the recruit form of the sweep takes no groups (clustering.neighbor_sweep
    # has the audit form only; the list form for new rows is Context.recruit_rows_multi, reached through _score_rows)
    dctx = _lib.default_context()
    with pytest.raises(ValueError, match="groups"):
        dctx._score_rows("recruit", labels, B, True, ms=[5, 3], Y=X[:8], groups=groups)
    with pytest.raises(ValueError, match="groups"):
        ctx.audit_rows_grouped(labels, groups[:-1], B, m)
    assert dctx.get_metric() == "convex"
