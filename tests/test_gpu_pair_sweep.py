"""chb_audit_pairs_multi / chb_recruit_pairs_multi and clustering.audit_pairs_sweep / recruit_pairs_sweep / cohesion_sweep: a
list of (row, bin) pairs scored for a list of m with entries up to 64, one selection pass per kernel family.

The calls are DEFINED by the single wide pair calls: slice j is bit for bit what chb_audit_pairs_wide /
chb_recruit_pairs_wide returns for m = ms[j].  Every comparison with a single call below is on the doubles' uint64 views,
NaN is asserted absent, no pair is left out and no tolerance applies.  One list is also held straight against the oracle
(row_reference.reference_rows and its bound), so that the new path does not lean on the single-m kernels alone."""
import numpy as np
import pytest

import row_reference
import wide_m_cases as W
from test_gpu_pairs import COUNTERS, bits, tiles_of

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
N, B, Q = W.N, W.B, W.Q
MS = (24, 5, 64, 17, 16, 33, 32, 1)   # unsorted, mixed, entries <= 32 beside max = 64: all three kernels in one call


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same(a, b):
    """bit for bit: the doubles as uint64, NaN nowhere"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64, (a.shape, b.shape, a.dtype, b.dtype)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert np.array_equal(bits(a), bits(b))


def grid(nrows, rng, step=1, repeat=True):
    """every (row, bin) of rows 0, step, 2 step, ... against all B bins, plus a fifth of them repeated, shuffled"""
    rows = np.repeat(np.arange(0, nrows, step, dtype=np.int64), B)
    bins = np.tile(np.arange(B, dtype=np.int64), len(rows) // B)
    if repeat:
        again = rng.integers(0, len(rows), len(rows) // 5)
        rows, bins = np.concatenate([rows, rows[again]]), np.concatenate([bins, bins[again]])
    order = rng.permutation(len(rows))
    return np.ascontiguousarray(rows[order]), np.ascontiguousarray(bins[order])


def check_audit(ctx, lab, ms, rows, bins, groups=None):
    got = ctx.audit_pairs_multi(lab, B, ms, rows, bins, groups=groups)
    assert got.shape == (len(ms), len(rows))
    for j, m in enumerate(ms):
        same(got[j], ctx.audit_pairs_wide(lab, B, m, rows, bins, groups=groups))
    return got


def check_recruit(ctx, lab, ms, Y, row_of, bins):
    got = ctx.recruit_pairs_multi(lab, B, ms, Y, row_of, bins)
    assert got.shape == (len(ms), len(row_of))
    for j, m in enumerate(ms):
        same(got[j], ctx.recruit_pairs_wide(lab, B, m, Y, row_of, bins))
    return got


# ---- 1. slices equal single calls

@pytest.mark.parametrize("D", [21, 72])
def test_slices_equal_single_calls(ctx, D):
    X, lab, Y, _ = W.wide(D, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(61)
    rows, bins = grid(N, rng, step=3)
    assert len(np.arange(0, N, 3)) == 234 == 3 * 64 + 42   # rows per bin before the repeats: three full tiles and one of 42
    got = check_audit(ctx, lab, MS, rows, bins)
    # ... and the matching entries of the dense list call
    scored = np.arange(0, N, 3, dtype=np.int64)
    dense = ctx.audit_rows_multi_wide(lab, B, MS, scored, want_dist=True)[1]
    same(got, np.ascontiguousarray(dense[:, rows // 3, bins]))
    # the list reached the kernels: neighbouring entries differ somewhere
    for a, b in ((16, 17), (32, 33), (33, 64)):
        assert not np.array_equal(bits(got[MS.index(a)]), bits(got[MS.index(b)]))
    # the +inf pattern: the empty bin, and nothing else but the lone member's own pair
    lone = int(np.flatnonzero(lab == 1)[0])
    want_inf = (bins == 0) | ((bins == 1) & (rows == lone))
    assert np.array_equal(np.isinf(got), np.tile(want_inf, (len(MS), 1))) and (got[:, want_inf] == np.inf).all()
    own = ctx.audit_pairs_multi(lab, B, MS, np.array([lone, lone]), np.array([1, 2]))
    assert np.all(own[:, 0] == np.inf) and np.isfinite(own[:, 1]).all()
    # recruit: every row of Y
    row_of, ybins = grid(Q, rng)
    rgot = check_recruit(ctx, lab, MS, Y, row_of, ybins)
    rdense = ctx.recruit_rows_multi_wide(lab, B, MS, Y, want_dist=True)[1]
    same(rgot, np.ascontiguousarray(rdense[:, row_of, ybins]))
    assert np.array_equal(np.isinf(rgot), np.tile(ybins == 0, (len(MS), 1)))
    for a, b in ((16, 17), (32, 33), (33, 64)):
        assert not np.array_equal(bits(rgot[MS.index(a)]), bits(rgot[MS.index(b)]))


# ---- 2. each kernel alone

@pytest.mark.parametrize("ms", [(1, 3, 5, 10, 15, 16), tuple(range(1, 17)), (17, 32, 20), (40,), (33,), (64, 33, 48), (3, 32),
                                (1,), (16,)], ids=lambda ms: "-".join(map(str, ms)))
def test_each_kernel_alone(ctx, ms):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(62)
    rows, bins = grid(N, rng, step=3)
    names = ("audit_pairs_multi", "audit_pairs_multi_wide_select", "audit_pairs_multi_wide_solve", "audit_pairs",
             "audit_pairs_wide_select", "audit_pairs_wide_solve", "audit_multi", "audit_multi_wide_select", "audit_multi_wide_solve")
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_pairs_multi(lab, B, ms, rows, bins)
    prof = {k: ctx.profile_get(k) for k in names}
    ctx.profile_enable(False)
    for j, m in enumerate(ms):
        same(got[j], ctx.audit_pairs_wide(lab, B, m, rows, bins))
    narrow, wide = sum(m <= 16 for m in ms), sum(m > 16 for m in ms)
    P = len(rows)
    assert prof["audit_pairs_multi"]["launches"] == (narrow > 0) and prof["audit_pairs_multi"]["work"] == P * narrow
    assert prof["audit_pairs_multi_wide_select"]["launches"] == (wide > 0) and prof["audit_pairs_multi_wide_select"]["work"] == P * (wide > 0)
    assert prof["audit_pairs_multi_wide_solve"]["launches"] == (wide > 0) and prof["audit_pairs_multi_wide_solve"]["work"] == P * wide
    for k in names[3:]:
        assert prof[k]["launches"] == 0, k
    row_of, ybins = grid(Q, rng, step=2)
    check_recruit(ctx, lab, ms, Y, row_of, ybins)


# ---- 3. the affine metric

def test_affine_metric(ctx):
    X, lab, Y, _ = W.wide(72, twins=0)
    ctx.set_samples(X)
    rng = np.random.default_rng(63)
    rows, bins = grid(N, rng, step=7)
    row_of, ybins = grid(Q, rng, step=2)
    ms = (33, 5, 64, 17, 24, 16)
    with ctx.using_metric("affine"):
        affine = check_audit(ctx, lab, ms, rows, bins)
        raffine = check_recruit(ctx, lab, ms, Y, row_of, ybins)
    convex = ctx.audit_pairs_multi(lab, B, ms, rows, bins)
    rconvex = ctx.recruit_pairs_multi(lab, B, ms, Y, row_of, ybins)
    for j in range(len(ms)):   # (the metric reached every kernel)
        assert not np.array_equal(bits(convex[j]), bits(affine[j])) and not np.array_equal(bits(rconvex[j]), bits(raffine[j]))


# ---- 4. groups

def test_groups(ctx):
    X, lab, _, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    groups = (np.random.default_rng(51).permutation(N) // 4).astype(np.int64)
    rows, bins = grid(N, np.random.default_rng(65), step=1, repeat=False)
    grouped = check_audit(ctx, lab, MS, rows, bins, groups=groups)
    plain = ctx.audit_pairs_multi(lab, B, MS, rows, bins)
    for j in range(len(MS)):
        assert not np.array_equal(bits(grouped[j]), bits(plain[j]))   # (siblings were among the nearest somewhere)
    check_audit(ctx, lab, (7, 12), rows[:500], bins[:500], groups=groups)   # (the grouped narrow kernel alone)


# ---- 5. the oracle

def test_against_the_oracle(ctx):
    D, ms = 72, (5, 17, 33)
    X, lab, _, _ = W.wide(D, twins=40)
    ctx.set_samples(X)
    rows, bins = grid(N, np.random.default_rng(66), repeat=False)   # (oracle_rows(17) is every row)
    got = ctx.audit_pairs_multi(lab, B, ms, rows, bins)
    table = np.full((len(ms), N, B), np.nan)
    table[:, rows, bins] = got
    for j, m in enumerate(ms):
        orows, ref = W.audit_reference(D, m, 40)
        assert np.array_equal(orows, W.oracle_rows(m))
        dist = table[j][orows]
        fin = np.isfinite(ref.dist)
        assert not np.isnan(dist).any()
        assert np.array_equal(np.isfinite(dist), fin) and np.array_equal(dist[~fin], ref.dist[~fin]), m
        err, bnd = np.abs(dist[fin] - ref.dist[fin]), row_reference.bound(ref)[fin]
        pos = bnd > 0
        print(f"list pairs D={D} m={m}: largest |d - oracle| / bound = {(err[pos] / bnd[pos]).max():.3e} over {fin.sum()} finite entries")
        assert np.all(err <= bnd), m


# ---- 6. chunks and tiles

def test_chunks_and_tiles(ctx):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(67)
    ms = (20, 3, 40, 16)
    rows1, bins1 = grid(N, rng, repeat=False)
    order = rng.permutation(4 * N * B)
    rows, bins = np.ascontiguousarray(np.tile(rows1, 4)[order]), np.ascontiguousarray(np.tile(bins1, 4)[order])
    assert len(rows) == 22400 > ctx.counter("recruit_chunk") == 16384
    names = ("audit_pairs_multi", "audit_pairs_multi_wide_select", "audit_pairs_multi_wide_solve")
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_pairs_multi(lab, B, ms, rows, bins)
    prof = {k: ctx.profile_get(k) for k in names}
    ctx.profile_enable(False)
    assert ctx.counter("pair_tiles") == tiles_of(bins, B)
    for k in names:
        assert prof[k]["launches"] == 2, k   # two chunks
    assert prof["audit_pairs_multi"]["work"] == 2 * len(rows) and prof["audit_pairs_multi_wide_select"]["work"] == len(rows)
    assert prof["audit_pairs_multi_wide_solve"]["work"] == 2 * len(rows)
    for j, m in enumerate(ms):
        same(got[j], ctx.audit_pairs_wide(lab, B, m, rows, bins))
        assert ctx.counter("pair_tiles") == tiles_of(bins, B)   # (the single call's value)
    once = ctx.audit_pairs_multi(lab, B, ms, rows1, bins1)
    same(got, np.ascontiguousarray(np.tile(once, (1, 4))[:, order]))   # (a repeated pair has the same bits in any chunk)
    # narrow entries only across two chunks, and the recruit form (a row of Y is packed once per pair)
    check_audit(ctx, lab, (15, 1, 5), rows, bins)
    row_of, ybins = rng.integers(0, Q, 17000), rng.integers(0, B, 17000)
    check_recruit(ctx, lab, ms, Y, row_of, ybins)
    assert ctx.counter("pair_tiles") == tiles_of(ybins, B)
    # one pair
    one = check_audit(ctx, lab, MS, np.array([5]), np.array([7]))
    assert ctx.counter("pair_tiles") == 1 and np.isfinite(one).all()
    check_recruit(ctx, lab, MS, Y, np.array([Q - 1]), np.array([3]))
    # all pairs in one bin: the tiles of a single run, the last one short
    rows7 = np.ascontiguousarray(rng.permutation(N)[:333].astype(np.int64))
    bins7 = np.full(333, 7, dtype=np.int64)
    check_audit(ctx, lab, MS, rows7, bins7)
    assert ctx.counter("pair_tiles") == 6 == tiles_of(bins7, B)
    # nothing to score
    empty = ctx.audit_pairs_multi(lab, B, (64, 20), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert empty.shape == (2, 0)


# ---- 7. refusals

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
        row_of = np.array([2, 0, 2], dtype=np.int64)
        bins = np.array([7, 2, 4], dtype=np.int64)
        mixed = (5, 40, 17)
        out = np.full(3 * 3, -77.0)
        KEEP = object()

        def audit(ms=mixed, nm=None, B_=B, rows_=rows, bins_=bins, P_=None, lab_=lab, out_=KEEP, h=KEEP):
            arr = None if ms is None else np.array(ms, dtype=np.intc)
            nm = (3 if ms is None else len(ms)) if nm is None else nm   # (a null list says it has three entries)
            return lib.chb_audit_pairs_multi(ctx._h if h is KEEP else h, ptr(lab_), None, B_, ptr(arr), nm, ptr(rows_), ptr(bins_),
                                             len(bins) if P_ is None else P_, ptr(out if out_ is KEEP else out_))

        def recruit(ms=mixed, nm=None, B_=B, rows_=row_of, bins_=bins, P_=None, lab_=lab, out_=KEEP, h=KEEP, D_=D, Q_=3, Y_=Y):
            arr = None if ms is None else np.array(ms, dtype=np.intc)
            nm = (3 if ms is None else len(ms)) if nm is None else nm
            return lib.chb_recruit_pairs_multi(ctx._h if h is KEEP else h, ptr(lab_), B_, ptr(arr), nm,
                                               ptr(Y_), Q_, D_, ptr(rows_), ptr(bins_), len(bins) if P_ is None else P_,
                                               ptr(out if out_ is KEEP else out_))

        def refused(rc, code, text=None):
            assert rc == code, (rc, code, lib.chb_last_error())
            if text:
                assert text in lib.chb_last_error().decode(), lib.chb_last_error()
            assert np.all(out == -77.0)

        bad_rows = np.array([3, N, 5], dtype=np.int64)
        bad_bins = np.array([7, B, -1], dtype=np.int64)
        # ---- a context without samples: checks 1 .. 8, each against the next one failing too
        for call in (audit, recruit):
            refused(call(h=None, P_=-1), EINVAL, "null context")                     # 1 before 2
            refused(call(P_=-1, ms=None), EINVAL, "Q < 0")                            # 2 before 3
            refused(call(B_=0, ms=None), EINVAL, "B < 1")
            refused(call(ms=None, nm=0), EINVAL, "ms is null")                        # 3 before 4
            refused(call(ms=(40, 0), nm=0), EINVAL, "nm")                             # 4 before 5
            refused(call(ms=tuple(range(17, 33)) + (0,), nm=17), EINVAL, "nm")
            refused(call(ms=(40, -3, 40)), EINVAL, "< 1")                             # 5 before 6
            refused(call(ms=(0, 5)), EINVAL, "< 1")
            refused(call(ms=(17, 17), lab_=None), EINVAL, "twice")                    # 6 before 7
            refused(call(ms=(64, 5, 33, 64), lab_=None), EINVAL, "twice")
            refused(call(ms=(5, 3, 5), lab_=None), EINVAL, "twice")
            refused(call(ms=(65, 17, 17), lab_=None), EINVAL, "twice")
            refused(call(lab_=None), EINVAL, "null")                                  # 7 before 8
            refused(call(rows_=None), EINVAL, "null")
            refused(call(bins_=None), EINVAL, "null")
            refused(call(out_=None), EINVAL, "null")
            refused(call(ms=(5, 65), B_=8193), ESTATE, "chb_set_samples")             # 8 before 10 and 12
        refused(recruit(Q_=-1, ms=None), EINVAL, "Q < 0")                             # 2 before 3, the rows of Y
        refused(recruit(Y_=None), EINVAL, "null")                                     # 7
        refused(recruit(D_=D + 1), ESTATE, "chb_set_samples")                         # 8 before 9
        ctx.set_samples(X)
        # ---- with samples: checks 9 .. 16
        refused(recruit(D_=D + 1, ms=(5, 65), B_=8193), EINVAL, "columns")            # 9 before 10
        for call in (audit, recruit):
            refused(call(lab_=None), EINVAL, "null")
            refused(call(out_=None), EINVAL, "null")
            refused(call(ms=(5, 65), B_=8193), EUNSUPPORTED, "at most 64 neighbours")   # 10 before 12
            refused(call(ms=(65,)), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(ms=(65, 65)), EUNSUPPORTED, "at most 64 neighbours")   # (an entry above 64 sets no bit: not "twice")
            refused(call(B_=8193, rows_=bad_rows), EUNSUPPORTED, "at most 8192 bins")   # 12 before 15
            refused(call(ms=(5, 3), B_=8193), EUNSUPPORTED, "at most 8192 bins")        # (without a wide entry too)
            refused(call(rows_=bad_rows, bins_=bad_bins), EINVAL, "row_idx" if call is audit else "row_of")   # 15 before 16
            refused(call(rows_=np.array([3, -1, 5], dtype=np.int64)), EINVAL, "row_idx" if call is audit else "row_of")
            refused(call(bins_=bad_bins), EINVAL, "bin_idx")                          # 16
            refused(call(bins_=np.array([7, 2, B], dtype=np.int64), ms=(3, 9)), EINVAL, "bin_idx")
            # 14. no pairs: fine, whatever the arrays, and nothing is read or written
            refused(call(P_=0, lab_=None, rows_=None, bins_=None, out_=None), 0)
            refused(call(P_=0, rows_=bad_rows, bins_=bad_bins), 0)
        refused(recruit(rows_=np.array([0, 3, 1], dtype=np.int64)), EINVAL, "row_of")   # (Q = 3 rows of Y)
        refused(recruit(P_=0, Y_=None, Q_=0, lab_=None, rows_=None, bins_=None, out_=None), 0)
        # ---- 13. an open stepwise fit: refused behind the limits, before P = 0 and the ranges, and the fit goes on
        Z, initial, _ = synth.make_synthetic(N, D, B, seed=3, sigma=6e-3, mix=0.5)
        ctx.set_samples(Z)
        sl = np.flatnonzero(initial == -1)[:100].astype(np.int64)

        def stepwise(with_calls):
            ctx.fit_begin(B, initial, 5)
            if with_calls:
                refused(audit(), ESTATE, "stepwise")
            ctx.batch_begin(sl, 0, len(sl))
            for call in (audit, recruit) if with_calls else ():
                refused(call(), ESTATE, "stepwise")
                refused(call(ms=(3, 9)), ESTATE, "stepwise")
                refused(call(rows_=bad_rows), ESTATE, "stepwise")                     # 13 before 15
                refused(call(P_=0), ESTATE, "stepwise")                               # 13 before 14
                refused(call(B_=8193), EUNSUPPORTED, "at most 8192 bins")             # 12 before 13
                refused(call(ms=(5, 65)), EUNSUPPORTED, "at most 64 neighbours")
            guess = np.full(len(sl), -1, dtype=np.int64)
            ctx.batch_guess(guess)
            lab1 = np.full(len(sl), -9, dtype=np.int64)
            ctx.batch_round(guess, 0, lab1)
            ctx.batch_commit(lab1)
            assert np.array_equal(ctx.fit_labels()[sl], lab1) and np.all(lab1 >= 0)
            return ctx.fit_labels()

        with_calls = stepwise(True)
        ctx.set_samples(Z)
        assert np.array_equal(with_calls, stepwise(False))   # (the labels it would have had)
        # chb_set_samples ends it; then the calls answer
        ctx.set_samples(X)
        assert audit() == 0 and np.isfinite(out).all()
        same(out.reshape(3, 3), ctx.audit_pairs_multi(lab, B, mixed, rows, bins))
        out[:] = -77.0
        assert recruit() == 0 and np.isfinite(out).all()
        same(out.reshape(3, 3), ctx.recruit_pairs_multi(lab, B, mixed, Y, row_of, bins))
    finally:
        ctx.close()


# ---- 8. the context is left as found

def test_no_trace_left_in_a_fit():
    from chbin_amd import _lib, synth
    Nf, D, Bf, m, its = 1500, 72, 6, 5, 3
    Z, initial, _ = synth.make_synthetic(Nf + 100, D, Bf, seed=41, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:Nf]), np.ascontiguousarray(Z[Nf:])
    initial = initial[:Nf].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    rng = np.random.default_rng(68)
    row_of, ybins = rng.integers(0, len(Y), 300), rng.integers(0, Bf, 300)

    def two_fits(calls_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(Bf, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in COUNTERS], ctx.fit_stats()))
                if k == 0 and calls_between:
                    assert ctx.counter("pair_tiles") == 0 and ctx.counter("recruit_wide_rows") == 0
                    rows = np.flatnonzero((lab >= 0) & (lab < Bf))
                    own = np.ascontiguousarray(lab[rows])
                    assert len(rows) > Nf // 2
                    a0 = ctx.audit_pairs_multi(lab, Bf, (1, 3, 5, 10, 15), rows, own)
                    assert ctx.counter("pair_tiles") == tiles_of(own, Bf) and ctx.counter("recruit_wide_rows") == 0
                    a1 = ctx.audit_pairs_multi(lab, Bf, (5, 24, 40), rows, own)
                    a2 = ctx.audit_pairs_multi(lab, Bf, (5, 24, 40), rows, own)
                    r1 = ctx.recruit_pairs_multi(lab, Bf, (64, 15, 33), Y, row_of, ybins)
                    r2 = ctx.recruit_pairs_multi(lab, Bf, (64, 15, 33), Y, row_of, ybins)
                    same(a1, a2)   # two identical calls, identical bits
                    same(r1, r2)
                    same(a0[2], a1[0])
                    assert np.isfinite(a0).any() and np.isfinite(a1).any() and np.isfinite(r1).any()
                    assert ctx.counter("pair_tiles") == tiles_of(ybins, Bf)
                    assert ctx.counter("recruit_wide_rows") == 16384   # (the single wide pair call's figure)
                    assert [ctx.counter(n) for n in COUNTERS] == res[0][3]
                    assert ctx.fit_stats() == res[0][4]
                    assert np.array_equal(ctx.fit_labels(), lab)
            return res
        finally:
            ctx.close()

    with_calls, without = two_fits(True), two_fits(False)
    for a, b in ((with_calls[0], with_calls[1]), (with_calls[1], without[1]), (with_calls[0], without[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert with_calls[1][3] == without[1][3] and with_calls[1][4] == without[1][4]


# ---- 9. the mirror

def test_mirror():
    from chbin_amd import clustering
    X, lab, Y, _ = W.wide(72, twins=0)
    labels = np.array(lab)
    labels[[4, 100]] = -1
    labels[[9, 333]] = (B, B + 5)
    groups = (np.random.default_rng(69).permutation(N) // 4).astype(np.int64)
    unscored = (labels < 0) | (labels >= B)

    def check_cohesion(ms, rows=None, **kw):
        got = clustering.cohesion_sweep(X, labels, B, **({} if ms is None else {"neighbors": ms}), rows=rows, **kw)
        ms = (1, 3, 5, 10, 15) if ms is None else ms
        out = unscored if rows is None else unscored[rows]
        assert got.shape == (len(ms), len(out)) and np.array_equal(np.isnan(got), np.tile(out, (len(ms), 1)))
        for j, m in enumerate(ms):
            want = clustering.cohesion(X, labels, B, num_neighbors=m, rows=rows, **kw)
            assert np.array_equal(np.isnan(want), out)
            same(got[j][~out], want[~out])
        return got

    full = check_cohesion(None)   # (the default list)
    assert np.isinf(full[:, labels == 1]).all() and np.isfinite(full[:, labels == 7]).all()
    rows = np.random.default_rng(70).integers(0, N, 150)
    rows[:4] = (4, 9, 100, 333)
    check_cohesion((5, 15, 24, 32, 64), rows)
    check_cohesion((40, 3), rows, groups=groups, metric="affine")
    # only each row's two nearest bins, against the dense sweep's entries
    ms = (1, 3, 5, 10, 15)
    near = clustering.nearest_bins(X, labels, B, k=2)
    pos, nbins = near.pairs()
    assert len(pos) == 2 * N and 2 * N < N * B
    sweep = clustering.neighbor_sweep(X, labels, B, ms, return_distances=True)
    got = clustering.audit_pairs_sweep(X, labels, pos, nbins, B)
    same(got, np.ascontiguousarray(sweep.distances[:, pos, nbins]))
    wide_ms = (15, 33, 2, 17)
    got = clustering.audit_pairs_sweep(X, labels, pos, nbins, B, neighbors=wide_ms, groups=groups)
    wsweep = clustering.neighbor_sweep_wide(X, labels, B, wide_ms, return_distances=True, groups=groups)
    same(got, np.ascontiguousarray(wsweep.distances[:, pos, nbins]))
    # the recruit form
    row_of, ybins = grid(Q, np.random.default_rng(71), step=3)
    got = clustering.recruit_pairs_sweep(X, labels, Y, row_of, ybins, B, neighbors=wide_ms, metric="affine")
    for j, m in enumerate(wide_ms):
        same(got[j], clustering.recruit_pairs(X, labels, Y, row_of, ybins, B, num_neighbors=m, metric="affine"))
    assert clustering.recruit_pairs_sweep(X, labels, Y, row_of, ybins, B).shape == (5, len(row_of))
