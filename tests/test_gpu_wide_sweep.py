"""chb_audit_rows_multi_wide / chb_recruit_rows_multi_wide / clustering.neighbor_sweep_wide: a list of m with entries up to
64 served from one selection pass per kernel family.

The calls are DEFINED by the single wide calls: slice j of every output is bit for bit what chb_audit_rows_wide /
chb_recruit_rows_wide returns for m = ms[j].  Every comparison with a single call below is on the doubles' uint64 views,
NaN is asserted absent, no case is left out and no tolerance applies.  One list is also held straight against the oracle
(test_gpu_wide_m.check_rows and its bound), so that the new path does not lean on the single-m kernels alone."""
import numpy as np
import pytest

import wide_m_cases as W
from test_gpu_pairs import COUNTERS, bits, tiles_of
from test_gpu_wide_m import check_rows, wide_rows

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
N, B, Q = W.N, W.B, W.Q
MS = (24, 5, 64, 17, 16, 33, 32, 1)   # unsorted, mixed, entries <= 32 beside max = 64: all three kernels in one call
# 16 entries, 9 of them wide: 1024 rows per chunk
MS16 = (64, 2, 33, 5, 17, 9, 32, 16, 20, 24, 40, 48, 1, 3, 12, 63)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same(a, b):
    """bit for bit: the doubles as uint64, NaN nowhere"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        assert not np.isnan(a).any() and not np.isnan(b).any()
        assert np.array_equal(bits(a), bits(b))
    else:
        assert np.array_equal(a, b)


def check_slices(multi, singles):
    """multi = (bins, dist or None, mind, margin) of a list call, singles[j] = the same of the single call for its entry j"""
    assert multi[0].shape[0] == len(singles)
    for j, one in enumerate(singles):
        for got, want in zip(multi, one):
            if got is None:
                assert want is None
            else:
                same(got[j], want)


# ---- 1. slices equal single calls

@pytest.mark.parametrize("D", [21, 72])
def test_slices_equal_single_calls(ctx, D):
    X, lab, Y, _ = W.wide(D, twins=40)
    ctx.set_samples(X)
    multi = ctx.audit_rows_multi_wide(lab, B, MS)
    singles = [ctx.audit_rows_wide(lab, B, m) for m in MS]
    assert multi[0].shape == (len(MS), N) and multi[1].shape == (len(MS), N, B)
    check_slices(multi, singles)
    check_slices(ctx.audit_rows_multi_wide(lab, B, MS, want_dist=False),
                 [ctx.audit_rows_wide(lab, B, m, want_dist=False) for m in MS])
    # the data does what it was made for: the empty bin, lists shorter than entries, entries that differ
    dist = multi[1]
    assert np.all(dist[:, :, 0] == np.inf) and np.isfinite(dist[:, :, 2:]).all()
    assert not np.array_equal(dist[MS.index(32)], dist[MS.index(33)]) and not np.array_equal(dist[MS.index(16)], dist[MS.index(17)])
    assert not np.array_equal(dist[MS.index(33)], dist[MS.index(64)])
    rmulti = ctx.recruit_rows_multi_wide(lab, B, MS, Y)
    assert rmulti[0].shape == (len(MS), Q) and rmulti[1].shape == (len(MS), Q, B)
    check_slices(rmulti, [ctx.recruit_rows_wide(lab, B, m, Y) for m in MS])
    check_slices(ctx.recruit_rows_multi_wide(lab, B, MS, Y, want_dist=False),
                 [ctx.recruit_rows_wide(lab, B, m, Y, want_dist=False) for m in MS])


# ---- 2. the 32-vertex form alone, the 64-vertex form alone, single-entry lists

@pytest.mark.parametrize("ms", [(17, 32, 20), (40,), (3, 32), (33,), (64, 33, 48)])
def test_the_32_vertex_form_and_short_lists(ctx, ms):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    check_slices(ctx.audit_rows_multi_wide(lab, B, ms), [ctx.audit_rows_wide(lab, B, m) for m in ms])
    check_slices(ctx.recruit_rows_multi_wide(lab, B, ms, Y), [ctx.recruit_rows_wide(lab, B, m, Y) for m in ms])


# ---- 3. the affine metric

def test_affine_metric(ctx):
    X, lab, Y, _ = W.wide(72, twins=0)
    ctx.set_samples(X)
    rows = np.arange(0, N, 7)
    ms = (33, 5, 64, 17, 24)
    with ctx.using_metric("affine"):
        multi = ctx.audit_rows_multi_wide(lab, B, ms, rows)
        singles = [ctx.audit_rows_wide(lab, B, m, rows) for m in ms]
        rmulti = ctx.recruit_rows_multi_wide(lab, B, ms, Y)
        rsingles = [ctx.recruit_rows_wide(lab, B, m, Y) for m in ms]
    check_slices(multi, singles)
    check_slices(rmulti, rsingles)
    convex = ctx.audit_rows_multi_wide(lab, B, ms, rows)
    assert not np.array_equal(bits(convex[1]), bits(multi[1]))   # (the metric reached the kernel)


# ---- 4. groups

def test_groups(ctx):
    X, lab, _, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    groups = (np.random.default_rng(51).permutation(N) // 4).astype(np.int64)
    grouped = ctx.audit_rows_multi_wide(lab, B, MS, groups=groups)
    check_slices(grouped, [ctx.audit_rows_wide(lab, B, m, groups=groups) for m in MS])
    plain = ctx.audit_rows_multi_wide(lab, B, MS)
    for j in range(len(MS)):
        assert not np.array_equal(bits(grouped[1][j]), bits(plain[1][j]))   # (siblings were among the nearest somewhere)
    rows = np.random.default_rng(52).integers(0, N, 90)
    check_slices(ctx.audit_rows_multi_wide(lab, B, (40, 7), rows, groups=groups),
                 [ctx.audit_rows_wide(lab, B, m, rows, groups=groups) for m in (40, 7)])


# ---- 5. the oracle

def test_against_the_oracle(ctx):
    D = 72
    X, lab, _, _ = W.wide(D, twins=0)
    ctx.set_samples(X)
    ms = (64, 5, 24)
    rows = np.arange(0, N, 7, dtype=np.int64)
    multi = ctx.audit_rows_multi_wide(lab, B, ms, rows)
    for m in (24, 64):
        rrows, ref = W.audit_reference(D, m, 0, every_seventh=True)
        assert np.array_equal(rrows, rows)
        check_rows([a[ms.index(m)] for a in multi], ref, f"list audit D={D} m={m}")


# ---- 6. chunks

def list_rows(width, ms):
    return min(wide_rows(width, max(ms)), max(64, 16384 // len(ms) // 64 * 64))


def test_chunks(ctx):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    nwide = sum(m > 16 for m in MS16)
    assert len(MS16) == 16 and nwide == 9
    one = ctx.audit_rows_multi_wide(lab, B, MS16)
    assert ctx.counter("recruit_wide_rows") == list_rows(B, MS16) == 1024
    rows = np.random.default_rng(53).integers(0, N, 1024 + 70)
    names = ("audit_multi_wide_select", "audit_multi_wide_solve", "audit_multi", "audit_wide_select", "audit_wide_solve",
             "audit", "recruit_multi_wide_select", "recruit_multi_wide_solve", "recruit_multi")
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_rows_multi_wide(lab, B, MS16, rows)
    prof = {k: ctx.profile_get(k) for k in names}
    ctx.profile_reset()
    only_wide = ctx.audit_rows_multi_wide(lab, B, (17, 64), rows)
    prof2 = {k: ctx.profile_get(k) for k in names}
    ctx.profile_reset()
    rgot = ctx.recruit_rows_multi_wide(lab, B, MS16, Y)
    prof3 = {k: ctx.profile_get(k) for k in names}
    ctx.profile_enable(False)
    for a, b in zip(got, one):
        same(a, np.ascontiguousarray(b[:, rows]))
    for k in ("audit_multi_wide_select", "audit_multi_wide_solve", "audit_multi"):
        assert prof[k]["launches"] == 2 and prof[k]["ms"] > 0.0
    assert prof["audit_multi_wide_select"]["work"] == len(rows) * B
    assert prof["audit_multi_wide_solve"]["work"] == len(rows) * B * nwide
    assert prof["audit_multi"]["work"] == len(rows) * B * (16 - nwide)
    for k in names[3:]:
        assert prof[k]["launches"] == 0, k
    assert ctx.counter("recruit_wide_rows") == 1024   # (the last call's: the recruit form, 16 entries again)
    # no narrow entry, no narrow launch; two entries, 8192 rows per chunk: one chunk
    assert prof2["audit_multi"]["launches"] == 0 and prof2["audit_multi_wide_select"]["launches"] == 1
    assert prof2["audit_multi_wide_solve"]["work"] == len(rows) * B * 2
    for j, m in enumerate((17, 64)):
        for a, b in zip(only_wide, one):
            same(a[j], np.ascontiguousarray(b[MS16.index(m)][rows]))
    # the recruit form books under its own names
    for k in ("recruit_multi_wide_select", "recruit_multi_wide_solve", "recruit_multi"):
        assert prof3[k]["launches"] == 1
    assert prof3["recruit_multi_wide_select"]["work"] == Q * B and prof3["recruit_multi_wide_solve"]["work"] == Q * B * nwide
    for k in names[:6]:
        assert prof3[k]["launches"] == 0, k
    check_slices(rgot, [ctx.recruit_rows_wide(lab, B, m, Y) for m in MS16])
    # many bins and a long list: the list buffer's bound is the smaller one
    few = np.arange(10)
    wide300 = ctx.audit_rows_multi_wide(lab, 300, (64, 20), few)
    assert ctx.counter("recruit_wide_rows") == min(3392, 8192) == list_rows(300, (64, 20))
    eight = ctx.audit_rows_multi_wide(lab, B, (64, 20), few)
    assert ctx.counter("recruit_wide_rows") == 8192
    same(np.ascontiguousarray(wide300[1][:, :, :B]), eight[1])
    assert np.all(wide300[1][:, :, B:] == np.inf)
    for k in (0, 2, 3):
        same(wide300[k], eight[k])
    # nothing to score
    empty = ctx.audit_rows_multi_wide(lab, B, (64, 20), np.zeros(0, dtype=np.int64))
    assert empty[0].shape == (2, 0) and empty[1].shape == (2, 0, B)
    empty = ctx.recruit_rows_multi_wide(lab, B, (64, 20), np.zeros((0, 21)))
    assert empty[0].shape == (2, 0) and empty[1].shape == (2, 0, B)


# ---- 7. lists without a wide entry forward

def test_narrow_lists_forward(ctx):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(54)
    groups = (rng.permutation(N) // 4).astype(np.int64)
    rows = rng.integers(0, N, 300)
    ctx.audit_rows_multi_wide(lab, B, (17, 3), rows)
    wide_before = ctx.counter("recruit_wide_rows")
    assert wide_before == 8192
    ctx.audit_rows_multi(lab, B, (1, 2, 3), rows)
    assert ctx.counter("recruit_multi_rows") == 5440
    ms = (5, 1, 16, 3, 8)
    got = ctx.audit_rows_multi_wide(lab, B, ms, rows)
    assert ctx.counter("recruit_multi_rows") == 16384 // 5 // 64 * 64 == 3264
    for a, b in zip(got, ctx.audit_rows_multi(lab, B, ms, rows)):
        same(a, b)
    for a, b in zip(ctx.audit_rows_multi_wide(lab, B, ms, rows, groups=groups), ctx.audit_rows_multi_grouped(lab, groups, B, ms, rows)):
        same(a, b)
    got = ctx.recruit_rows_multi_wide(lab, B, (16, 2, 9), Y)
    assert ctx.counter("recruit_multi_rows") == 5440
    for a, b in zip(got, ctx.recruit_rows_multi(lab, B, (16, 2, 9), Y)):
        same(a, b)
    assert ctx.counter("recruit_wide_rows") == wide_before
    # a wide list leaves the list calls' counter alone
    ctx.audit_rows_multi_wide(lab, B, (17, 3, 4, 5, 6), rows)
    assert ctx.counter("recruit_multi_rows") == 5440 and ctx.counter("recruit_wide_rows") == 3264


# ---- 8. refusals

def ptr(a):
    return None if a is None else a.ctypes.data


def test_refusals():
    from chbin_amd import _lib, synth
    lib = _lib.load()
    D = 21
    X, lab, Y, _ = W.wide(D, twins=0)
    lab = np.ascontiguousarray(lab)
    Y = np.ascontiguousarray(Y[:3])
    ctx = _lib.Context(0)
    try:
        rows = np.array([3, 5, 699], dtype=np.int64)
        wide = (5, 40, 17)
        out = {k: np.full(3 * 3 * B, -77.0) for k in ("dist", "min", "margin")}
        obin = np.full(3 * 3, -77, dtype=np.int64)

        def audit(ms=wide, nm=None, B_=B, rows_=rows, Q_=None, lab_=lab, sym=lib.chb_audit_rows_multi_wide, bin_=obin, dist_=out["dist"]):
            arr = None if ms is None else np.array(ms, dtype=np.intc)
            head = (ptr(lab_), None) if sym is lib.chb_audit_rows_multi_wide else (ptr(lab_),)
            return sym(ctx._h, *head, B_, ptr(arr), len(ms) if nm is None else nm, ptr(rows_),
                       (0 if rows_ is None else len(rows_)) if Q_ is None else Q_, ptr(bin_), ptr(dist_), ptr(out["min"]), ptr(out["margin"]))

        def recruit(ms=wide, nm=None, B_=B, D_=D, Q_=3, Y_=Y, sym=lib.chb_recruit_rows_multi_wide):
            arr = None if ms is None else np.array(ms, dtype=np.intc)
            return sym(ctx._h, ptr(lab), B_, ptr(arr), len(ms) if nm is None else nm, ptr(Y_), Q_, D_, ptr(obin),
                       ptr(out["dist"]), ptr(out["min"]), ptr(out["margin"]))

        def untouched():
            return all(np.all(a == -77.0) for a in out.values()) and np.all(obin == -77)

        def refused(rc, code, text=None):
            assert rc == code, (rc, lib.chb_last_error())
            if text:
                assert text in lib.chb_last_error().decode()
            assert untouched()

        # no samples: behind the list's own checks, the null arguments and the outputs; before D, the limits and B
        refused(audit(), ESTATE)
        refused(recruit(ms=(5, 65), D_=D + 1, B_=8193), ESTATE)
        refused(audit(ms=(17, 17)), EINVAL, "twice")
        refused(audit(lab_=None), EINVAL, "null")
        refused(audit(bin_=None, dist_=None), EINVAL, "both null")
        ctx.set_samples(X)
        for call in (audit, recruit):
            # 1. ranges, before the list is read
            refused(call(Q_=-1, ms=(40, 0)), EINVAL, "Q < 0")
            refused(call(B_=0, ms=None, nm=2), EINVAL, "B < 1")
            # 2. ms null, 3. nm, 4. an entry < 1, 5. a repeated entry
            refused(call(ms=None, nm=2), EINVAL, "ms is null")
            refused(call(nm=0), EINVAL, "nm")
            refused(call(ms=tuple(range(17, 34)), nm=17), EINVAL, "nm")
            refused(call(ms=(40, 0)), EINVAL, "< 1")
            refused(call(ms=(40, -3, 40)), EINVAL, "< 1")
            refused(call(ms=(17, 17)), EINVAL, "twice")
            refused(call(ms=(64, 5, 33, 64)), EINVAL, "twice")
            refused(call(ms=(5, 40, 5), B_=8193), EINVAL, "twice")
            refused(call(ms=(65, 17, 17)), EINVAL, "twice")
            # 7. more than 64 (an entry above 64 sets no bit: two of them are not "twice"), before 9. the bins
            refused(call(ms=(5, 65)), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(ms=(65, 65)), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(ms=(5, 65), B_=8193), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(B_=8193), EUNSUPPORTED, "at most 8192 bins")
        # 6. D before the limits
        refused(recruit(D_=D + 1, ms=(5, 65), B_=8193), EINVAL, "columns")
        refused(recruit(Y_=None), EINVAL, "null")
        refused(audit(lab_=None), EINVAL, "null")
        refused(audit(bin_=None, dist_=None), EINVAL, "both null")
        # 12. the row_idx rules
        refused(audit(rows_=np.array([3, N, 5], dtype=np.int64)), EINVAL, "row_idx")
        refused(audit(rows_=np.array([3, -1, 5], dtype=np.int64)), EINVAL, "row_idx")
        refused(audit(rows_=None, Q_=3), EINVAL, "row_idx is null")
        # the narrow symbols keep their limit and their texts
        refused(audit(ms=(5, 17, 2), sym=lib.chb_audit_rows_multi), EUNSUPPORTED, "chb_audit_rows_multi supports at most 16 neighbours")
        refused(recruit(ms=(5, 17, 2), sym=lib.chb_recruit_rows_multi), EUNSUPPORTED, "chb_recruit_rows_multi supports at most 16")
        refused(audit(ms=(5, 17, 17), sym=lib.chb_audit_rows_multi), EUNSUPPORTED, "at most 16 neighbours")
        # ... which a forwarded list's refusals carry too
        refused(audit(ms=(5, 5)), EINVAL, "twice")
        refused(audit(ms=(5, 3), B_=8193), EUNSUPPORTED, "chb_audit_rows_multi supports at most 8192 bins")
        # an open stepwise fit: refused, and the fit goes on
        Z, initial, _ = synth.make_synthetic(N, D, B, seed=3, sigma=6e-3, mix=0.5)
        ctx.set_samples(Z)
        sl = np.flatnonzero(initial == -1)[:100].astype(np.int64)
        ctx.fit_begin(B, initial, 5)
        refused(audit(), ESTATE, "stepwise")
        ctx.batch_begin(sl, 0, len(sl))
        for call in (audit, recruit):
            refused(call(), ESTATE, "stepwise")
            refused(call(ms=(5, 65)), EUNSUPPORTED, "at most 64 neighbours")   # (the limits come first)
        guess = np.full(len(sl), -1, dtype=np.int64)
        ctx.batch_guess(guess)
        lab1 = np.full(len(sl), -9, dtype=np.int64)
        ctx.batch_round(guess, 0, lab1)
        ctx.batch_commit(lab1)
        assert np.array_equal(ctx.fit_labels()[sl], lab1) and np.all(lab1 >= 0)
        # chb_set_samples ends it; 11. Q = 0 is fine and writes nothing; then the calls answer
        ctx.set_samples(X)
        refused(audit(rows_=np.zeros(0, dtype=np.int64)), 0)
        refused(recruit(Q_=0), 0)
        assert audit() == 0 and np.all(obin >= 0) and np.isfinite(out["dist"]).sum() > 0 and not np.isnan(out["dist"]).any()
        assert recruit() == 0
    finally:
        ctx.close()


# ---- 9. the context is left as found

def test_no_trace_left_in_a_fit():
    from chbin_amd import _lib, synth
    Nf, D, Bf, m, its = 1500, 72, 6, 5, 3
    Z, initial, _ = synth.make_synthetic(Nf + 100, D, Bf, seed=41, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:Nf]), np.ascontiguousarray(Z[Nf:])
    initial = initial[:Nf].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    counters = COUNTERS + ("pair_tiles",)

    def two_fits(wide_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(Bf, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in counters], ctx.fit_stats()))
                if k == 0 and wide_between:
                    assert ctx.counter("recruit_wide_rows") == 0
                    a1 = ctx.audit_rows_multi_wide(lab, Bf, (5, 24, 40))
                    a2 = ctx.audit_rows_multi_wide(lab, Bf, (5, 24, 40))
                    r1 = ctx.recruit_rows_multi_wide(lab, Bf, (64, 15, 33), Y)
                    r2 = ctx.recruit_rows_multi_wide(lab, Bf, (64, 15, 33), Y)
                    for x, y in zip(a1 + r1, a2 + r2):   # two identical calls, identical bits
                        same(x, y)
                    assert np.isfinite(a1[2]).all() and np.isfinite(r1[2]).all()
                    assert ctx.counter("recruit_wide_rows") == 16384 // 3 // 64 * 64
                    assert [ctx.counter(n) for n in counters] == res[0][3]
                    assert ctx.fit_stats() == res[0][4]
                    assert np.array_equal(ctx.fit_labels(), lab)
            return res
        finally:
            ctx.close()

    with_calls, without = two_fits(True), two_fits(False)
    for a, b in ((with_calls[0], with_calls[1]), (with_calls[1], without[1]), (with_calls[0], without[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert with_calls[1][3] == without[1][3] and with_calls[1][4] == without[1][4]


# ---- 10. the mirror

def test_mirror():
    from chbin_amd import clustering
    X, lab, _, _ = W.wide(72, twins=0)
    ms = (5, 15, 24, 32, 64)

    def check(sweep, rows, **kw):
        scored = np.arange(N) if rows is None else np.asarray(rows)
        assert np.array_equal(sweep.neighbors, ms) and np.array_equal(sweep.rows, scored) and np.array_equal(sweep.own, lab[scored])
        assert sweep.num_clusters == B
        for j, m in enumerate(ms):
            bins, mind, margin, dist = clustering.audit(X, lab, B, num_neighbors=m, rows=rows, return_distances=True, **kw)
            same(sweep.bins[j], bins)
            same(sweep.min_dist[j], mind)
            same(sweep.margin[j], margin)
            same(sweep.distances[j], dist)
        labelled = (sweep.own >= 0) & (sweep.own < B)
        assert np.array_equal(sweep.moved, ((sweep.bins != sweep.own[None, :]) & labelled[None, :]).sum(axis=1))
        agree = (sweep.bins[:, None, :] == sweep.bins[None, :, :]).mean(axis=2)
        assert np.array_equal(sweep.agreement, agree)
        assert np.array_equal(sweep.stable(0.01), labelled & np.all((sweep.bins == sweep.own[None, :]) & (sweep.margin > 0.01), axis=0))

    full = clustering.neighbor_sweep_wide(X, lab, B, return_distances=True)
    assert tuple(full.neighbors) == ms   # (the default list)
    check(full, None)
    assert full.stable().any() and full.moved.max() > 0 and clustering.neighbor_sweep_wide(X, lab, B).distances is None
    rows = np.random.default_rng(55).integers(0, N, 120)
    groups = (np.random.default_rng(56).permutation(N) // 4).astype(np.int64)
    check(clustering.neighbor_sweep_wide(X, lab, B, ms, rows=rows, return_distances=True, groups=groups), rows, groups=groups)
    check(clustering.neighbor_sweep_wide(X, lab, B, ms, metric="affine", rows=rows, return_distances=True), rows, metric="affine")
