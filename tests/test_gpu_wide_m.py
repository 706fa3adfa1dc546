"""chb_audit_rows_wide / chb_recruit_rows_wide / chb_audit_pairs_wide / chb_recruit_pairs_wide: row scoring for
16 < m <= 64 (two kernels per chunk, recruit_wide_kernels.hip), and the forwarding of m <= 16.

Yardsticks: the selection lists against chb_topm_per_bin and the oracle's sets, exactly; the distances against
row_reference (the oracle on the shifted problem, inside the envelope test_wide_m_cpu.py checks it keeps on this data)
within row_reference.bound, and against chb_hull_distance_batch on the same lists -- the same driver on another Gram
arithmetic -- within the same bound; everything else bitwise (uint64 views) against the dense wide call itself."""
import numpy as np
import pytest

import row_reference
import wide_m_cases as W
from test_gpu_pairs import COUNTERS, bits, tiles_of

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
N, B, Q = W.N, W.B, W.Q


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def grid(rng):
    """every (row, bin) pair of the N x B grid, shuffled"""
    order = rng.permutation(N * B)
    return order // B, order % B, order


_LISTS = {}


def lists_of(ctx, D, m, twins):
    """(rows, bins, idx [N * B, m], dist [N * B]) of audit_pairs_wide over the whole grid in grid order (scored shuffled),
    once per case"""
    key = (D, m, twins)
    if key not in _LISTS:
        X, lab, _, _ = W.wide(D, twins=twins)
        ctx.set_samples(X)
        rows, bins, order = grid(np.random.default_rng(31))
        dist, idx = ctx.audit_pairs_wide(lab, B, m, rows, bins, want_idx=True)
        back = np.argsort(order)
        _LISTS[key] = (rows[back], bins[back], idx[back], dist[back])
    return _LISTS[key]


# ---- 1. the selection is exact

@pytest.mark.parametrize("twins", [0, 40])
@pytest.mark.parametrize("D", [21, 72])
@pytest.mark.parametrize("m", [17, 32, 33, 48, 64])
def test_selection_is_exact(ctx, m, D, twins):
    X, lab, Y, _ = W.wide(D, twins=twins)
    rows, bins, idx, _ = lists_of(ctx, D, m, twins)
    assert idx.dtype == np.int64 and idx.shape == (N * B, m)
    want, _, cnt = ctx.topm_per_bin(lab, B, m, np.arange(N))
    assert np.array_equal(idx.reshape(N, B, m), want)
    assert np.array_equal((idx >= 0).sum(axis=1).reshape(N, B), cnt)
    assert cnt.max() == m and cnt.min() == 0   # a full list, and the empty bin / the lone member's own pair
    # rows that are not samples: against the oracle's sets
    ctx.set_samples(X)
    ref = W.recruit_reference(D, m, twins)
    order = np.random.default_rng(32).permutation(Q * B)
    got = ctx.recruit_pairs_wide(lab, B, m, Y, order // B, order % B, want_idx=True)[1]
    assert np.array_equal(got[np.argsort(order)].reshape(Q, B, m)[W.YROWS], W.padded_sets(ref.sets, m))


# ---- 2. distances against the oracle

def check_rows(got, ref, what):
    bins, dist, mind, margin = got
    fin = np.isfinite(ref.dist)
    assert np.array_equal(np.isfinite(dist), fin) and np.array_equal(dist[~fin], ref.dist[~fin]), what
    err, bnd = np.abs(dist[fin] - ref.dist[fin]), row_reference.bound(ref)[fin]
    pos = bnd > 0   # (a problem whose vertices all coincide with the row has scale 0: exact or failed)
    print(f"{what}: largest |d - oracle| / bound = {(err[pos] / bnd[pos]).max():.3e} over {fin.sum()} finite entries")
    assert np.all(err <= bnd), what
    best, clear = row_reference.clear_rows(ref)
    assert clear.all() and np.array_equal(bins, best), what
    # the reduction is consistent with the table, bitwise
    b2, second = row_reference.strict_argmin(dist)
    q = np.arange(len(dist))
    assert np.array_equal(bins, b2)
    has = bins >= 0
    assert np.array_equal(bits(mind[has]), bits(dist[q[has], bins[has]])) and np.all(mind[~has] == np.inf)
    has2 = second >= 0
    assert np.array_equal(bits(margin[has2]), bits(dist[q[has2], second[has2]] - mind[has2])) and np.all(margin[~has2] == np.inf)


@pytest.mark.parametrize("D,m", [(72, 17), (72, 33), (72, 64), (21, 17)])
def test_distances_match_the_oracle(ctx, D, m):
    twins = 40
    X, lab, Y, pairs = W.wide(D, twins=twins)
    ctx.set_samples(X)
    rows, ref = W.audit_reference(D, m, twins)
    got = ctx.audit_rows_wide(lab, B, m, rows)
    check_rows(got, ref, f"audit D={D} m={m}")
    check_rows([a[W.YROWS] for a in ctx.recruit_rows_wide(lab, B, m, Y)], W.recruit_reference(D, m, twins), f"recruit D={D} m={m}")
    # a twin's pair is exactly 0, also where the bin is the row's own; the lone member's own pair is +inf
    pr = np.array([t for t, s in pairs] + [s for t, s in pairs])
    pb = lab[np.array([s for t, s in pairs] + [t for t, s in pairs])]
    assert len(pr) == 80 and np.all(ctx.audit_pairs_wide(lab, B, m, pr, pb) == 0.0)
    lone = np.flatnonzero(lab == 1)
    assert len(lone) == 1
    assert ctx.audit_pairs_wide(lab, B, m, lone, [1])[0] == np.inf
    assert np.all(ctx.audit_rows_wide(lab, B, m)[1][:, 0] == np.inf)   # the bin without a member


# ---- 3. distances against the existing route on the same lists

@pytest.mark.parametrize("twins", [0, 40])
@pytest.mark.parametrize("D", [21, 72])
@pytest.mark.parametrize("m", [17, 33, 64])
def test_distances_match_hull_distance_batch(ctx, m, D, twins):
    X, lab, _, _ = W.wide(D, twins=twins)
    rows, bins, idx, dist = lists_of(ctx, D, m, twins)
    ctx.set_samples(X)
    some = np.flatnonzero(idx[:, 0] >= 0)
    assert np.all(dist[idx[:, 0] < 0] == np.inf) and np.isfinite(dist[some]).all()
    some = some[np.random.default_rng(33).permutation(len(some))[:1500]]   # (the composed route is slow by design)
    other = ctx.hull_distance_batch(rows[some], idx[some])
    P = X[np.maximum(idx[some], 0)] - X[rows[some]][:, None, :]
    scale = np.where(idx[some] >= 0, np.sqrt((P * P).sum(axis=2)), 0.0).max(axis=1)
    ref = row_reference.RowReference(other.reshape(-1, 1), scale.reshape(-1, 1), None)
    err, bnd = np.abs(dist[some] - other), row_reference.bound(ref)[:, 0]
    print(f"D={D} m={m} twins={twins}: largest |wide - batch| / bound = {(err / bnd).max():.3e}")
    assert np.all(err <= bnd)


# ---- 4. the affine metric

@pytest.mark.parametrize("m", [17, 33, 64])
def test_affine_metric(ctx, m):
    from oracle import oracle as O
    D = 72
    X, lab, _, _ = W.wide(D, twins=0)
    ctx.set_samples(X)
    rows = np.arange(0, N, 7)
    _, ref = W.audit_reference(D, m, 0, every_seventh=True)   # (the sets and the scales: the selection knows no metric)
    with ctx.using_metric("affine"):
        _, dist, _, _ = ctx.audit_rows_wide(lab, B, m, rows)
    want = np.full(dist.shape, np.inf)
    zero = np.zeros(D)
    for q, r in enumerate(rows):
        for c in range(B):
            if len(ref.sets[q][c]):
                want[q, c] = O.affine_hull_distance(zero, np.ascontiguousarray(X[ref.sets[q][c]] - X[r]))
    aref = row_reference.RowReference(want, ref.scale, None)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(dist), fin)
    err, bnd = np.abs(dist[fin] - want[fin]), row_reference.bound(aref)[fin]
    print(f"affine m={m}: largest |d - oracle| / bound = {(err / bnd).max():.3e}")
    assert np.all(err <= bnd)


# ---- 5. pairs equal dense, bitwise

@pytest.mark.parametrize("D,m", [(21, 17), (72, 33), (21, 48), (72, 64)])
def test_pairs_equal_dense_bitwise(ctx, D, m):
    X, lab, Y, _ = W.wide(D, twins=40)
    rows, bins, _, dist = lists_of(ctx, D, m, 40)
    ctx.set_samples(X)
    dense = ctx.audit_rows_wide(lab, B, m)[1]
    assert np.array_equal(bits(dist), bits(dense[rows, bins]))   # every pair of the grid, scored shuffled
    rng = np.random.default_rng(34)
    sub = rng.choice(N * B, N * B // 10, replace=False)
    sub = np.concatenate([sub, sub[: len(sub) // 5]])[rng.permutation(len(sub) + len(sub) // 5)]
    r, b = sub // B, sub % B
    assert np.array_equal(bits(ctx.audit_pairs_wide(lab, B, m, r, b)), bits(dense[r, b]))
    assert ctx.counter("pair_tiles") == tiles_of(b, B)
    rdense = ctx.recruit_rows_wide(lab, B, m, Y)[1]
    order = rng.permutation(Q * B)
    assert np.array_equal(bits(ctx.recruit_pairs_wide(lab, B, m, Y, order // B, order % B)), bits(rdense[order // B, order % B]))
    assert ctx.counter("pair_tiles") == B * ((Q + 63) // 64)


# ---- 6. groups

@pytest.mark.parametrize("m", [17, 64])
def test_groups(ctx, m):
    X, lab, _, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(35)
    groups = (rng.permutation(N) // 4).astype(np.int64) * 1000 + 7   # four-piece parents, ids neither dense nor small
    groups[rng.permutation(N)[:100]] = -3                           # ... and samples without a group
    plain = ctx.audit_rows_wide(lab, B, m)
    grouped = ctx.audit_rows_wide(lab, B, m, groups=groups)
    free = groups < 0
    for a, b in zip(grouped, plain):   # a negative group withholds nothing
        assert np.array_equal(bits(a[free]) if a.dtype != np.int64 else a[free], bits(b[free]) if b.dtype != np.int64 else b[free])
    picked = np.flatnonzero(~free)[rng.permutation(np.count_nonzero(~free))[:10]]
    differs = 0
    for r in picked:
        cut = lab.copy()
        cut[groups == groups[r]] = -1
        want = ctx.audit_rows_wide(cut, B, m, [r])
        for a, b in zip(grouped, want):
            assert np.array_equal(bits(a[r:r + 1]) if a.dtype != np.int64 else a[r:r + 1], bits(b) if b.dtype != np.int64 else b)
        differs += not np.array_equal(bits(grouped[1][r]), bits(plain[1][r]))
        pr, pb = np.full(B, r), np.arange(B)
        assert np.array_equal(bits(ctx.audit_pairs_wide(lab, B, m, pr, pb, groups=groups)), bits(grouped[1][r]))
    assert differs > 0   # (the siblings were among the nearest members somewhere)


# ---- 7. chunks

def wide_rows(width, m):
    return min(16384, max(64, (256 << 20) // (width * (m + 1) * 4) // 64 * 64))


def test_chunks(ctx):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    m = 17
    one = ctx.audit_rows_wide(lab, B, m)
    assert ctx.counter("recruit_wide_rows") == wide_rows(B, m) == 16384
    rows = np.random.default_rng(36).integers(0, N, 16384 + 70)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_rows_wide(lab, B, m, rows)
    prof = {k: ctx.profile_get(k) for k in ("audit_wide_select", "audit_wide_solve", "audit", "recruit_wide_select")}
    ctx.profile_enable(False)
    for a, b in zip(got, one):
        assert np.array_equal(bits(a) if a.dtype != np.int64 else a, bits(b[rows]) if b.dtype != np.int64 else b[rows])
    for k in ("audit_wide_select", "audit_wide_solve"):
        assert prof[k]["launches"] == 2 and prof[k]["work"] == len(rows) * B and prof[k]["ms"] > 0.0
    assert prof["audit"]["launches"] == 0 and prof["recruit_wide_select"]["launches"] == 0
    # a pair list across the chunk boundary
    p = np.arange(16384 + 70)
    pr, pb = p % N, (p // 7) % B
    assert np.array_equal(bits(ctx.audit_pairs_wide(lab, B, m, pr, pb)), bits(one[1][pr, pb]))
    assert ctx.counter("pair_tiles") == tiles_of(pb, B) and ctx.counter("recruit_wide_rows") == 16384
    # many bins and a long list: the chunk drops below 16384 rows, and three chunks give what one gives
    few = np.arange(10)
    wide300 = ctx.audit_rows_wide(lab, 300, 64, few)
    assert ctx.counter("recruit_wide_rows") == wide_rows(300, 64) == 3392
    assert np.array_equal(bits(wide300[1][:, :B]), bits(ctx.audit_rows_wide(lab, B, 64, few)[1]))
    assert np.all(wide300[1][:, B:] == np.inf)
    assert ctx.counter("recruit_wide_rows") == wide_rows(B, 64) == 16384
    # nothing to score
    tiles = ctx.counter("pair_tiles")
    empty = ctx.audit_rows_wide(lab, B, m, np.zeros(0, dtype=np.int64))
    assert empty[0].shape == (0,) and empty[1].shape == (0, B)
    assert ctx.recruit_rows_wide(lab, B, m, np.zeros((0, 21)))[1].shape == (0, B)
    assert ctx.audit_pairs_wide(lab, B, m, [], []).shape == (0,)
    d, i = ctx.recruit_pairs_wide(lab, B, m, Y, [], [], want_idx=True)
    assert d.shape == (0,) and i.shape == (0, m) and ctx.counter("pair_tiles") == tiles


# ---- 8. m <= 16 forwards

@pytest.mark.parametrize("m", [1, 15, 16])
def test_small_m_forwards(ctx, m):
    X, lab, Y, _ = W.wide(21, twins=40)
    ctx.set_samples(X)
    rng = np.random.default_rng(37)
    groups = (rng.permutation(N) // 4).astype(np.int64)
    rows = rng.integers(0, N, 300)
    pb = rng.integers(0, B, 300)
    row_of = rng.integers(0, Q, 300)

    def same(got, want):
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a if a.dtype == np.int64 else bits(a), b if b.dtype == np.int64 else bits(b))

    wide_before = ctx.counter("recruit_wide_rows")
    same(ctx.audit_rows_wide(lab, B, m, rows), ctx.audit_rows(lab, B, m, rows))
    same(ctx.audit_rows_wide(lab, B, m, rows, groups=groups), ctx.audit_rows_grouped(lab, groups, B, m, rows))
    same(ctx.recruit_rows_wide(lab, B, m, Y), ctx.recruit_rows(lab, B, m, Y))
    same([ctx.audit_pairs_wide(lab, B, m, rows, pb)], [ctx.audit_pairs(lab, B, m, rows, pb)])
    same([ctx.audit_pairs_wide(lab, B, m, rows, pb, groups=groups)], [ctx.audit_pairs_grouped(lab, groups, B, m, rows, pb)])
    same([ctx.recruit_pairs_wide(lab, B, m, Y, row_of, pb)], [ctx.recruit_pairs(lab, B, m, Y, row_of, pb)])
    same(ctx.audit_pairs_wide(lab, B, m, rows, pb, groups=groups, want_idx=True),
         ctx.audit_pairs_witness(lab, B, m, rows, pb, groups=groups)[:2])
    same(ctx.recruit_pairs_wide(lab, B, m, Y, row_of, pb, want_idx=True), ctx.recruit_pairs_witness(lab, B, m, Y, row_of, pb)[:2])
    assert ctx.counter("recruit_wide_rows") == wide_before


# ---- 9. refusals

def ptr(a):
    return None if a is None else a.ctypes.data


def test_refusals():
    from chbin_amd import _lib, synth
    lib = _lib.load()
    D, m = 21, 17
    X, lab, Y, _ = W.wide(D, twins=0)
    lab = np.ascontiguousarray(lab)
    ctx = _lib.Context(0)
    try:
        rows = np.array([3, 5, 699], dtype=np.int64)
        pbins = np.array([1, 7, 4], dtype=np.int64)
        row_of = np.array([0, 199, 7], dtype=np.int64)
        out = {k: np.full(3 * B, -77.0) for k in ("dist", "min", "margin")}
        obin, oidx = np.full(3, -77, dtype=np.int64), np.full(3 * 65, -77, dtype=np.int64)

        def audit(B_=B, m_=m, rows_=rows, lab_=lab):
            return lib.chb_audit_rows_wide(ctx._h, ptr(lab_), None, B_, m_, ptr(rows_), len(rows_), ptr(obin), ptr(out["dist"]),
                                           ptr(out["min"]), ptr(out["margin"]))

        def recruit(B_=B, m_=m, D_=D):
            return lib.chb_recruit_rows_wide(ctx._h, ptr(lab), B_, m_, ptr(Y), 3, D_, ptr(obin), ptr(out["dist"]),
                                             ptr(out["min"]), ptr(out["margin"]))

        def apairs(B_=B, m_=m, rows_=rows, bins_=pbins):
            return lib.chb_audit_pairs_wide(ctx._h, ptr(lab), None, B_, m_, ptr(rows_), ptr(bins_), 3, ptr(out["dist"]), ptr(oidx))

        def rpairs(B_=B, m_=m, D_=D, row_of_=row_of, bins_=pbins):
            return lib.chb_recruit_pairs_wide(ctx._h, ptr(lab), B_, m_, ptr(Y), Q, D_, ptr(row_of_), ptr(bins_), 3,
                                              ptr(out["dist"]), ptr(oidx))

        def untouched():
            return all(np.all(a == -77.0) for a in out.values()) and np.all(obin == -77) and np.all(oidx == -77)

        def refused(rc, code, text=None):
            assert rc == code, (rc, lib.chb_last_error())
            if text:
                assert text in lib.chb_last_error().decode()
            assert untouched()

        # no samples: before D, m and B
        refused(audit(), ESTATE)
        refused(recruit(D_=D + 1, m_=65, B_=8193), ESTATE)
        ctx.set_samples(X)
        # D before m, m before B; each on its own
        refused(recruit(D_=D + 1, m_=65), EINVAL)
        refused(rpairs(D_=D - 1, B_=8193), EINVAL)
        for call in (audit, recruit, apairs, rpairs):
            refused(call(m_=65, B_=8193), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(B_=8193), EUNSUPPORTED, "at most 8192 bins")
            refused(call(m_=0), EINVAL)
        # entries out of range
        refused(audit(rows_=np.array([3, N, 5], dtype=np.int64)), EINVAL, "row_idx")
        refused(apairs(rows_=np.array([3, -1, 5], dtype=np.int64)), EINVAL, "row_idx")
        refused(apairs(bins_=np.array([1, B, 4], dtype=np.int64)), EINVAL, "bin_idx")
        refused(rpairs(bins_=np.array([-1, 0, 4], dtype=np.int64)), EINVAL, "bin_idx")
        refused(rpairs(row_of_=np.array([0, Q, 7], dtype=np.int64)), EINVAL, "row_of")
        # the old entry points keep their limit
        assert lib.chb_audit_rows(ctx._h, ptr(lab), B, 17, ptr(rows), 3, ptr(obin), ptr(out["dist"]), None, None) == EUNSUPPORTED
        assert "at most 16 neighbours" in lib.chb_last_error().decode()
        assert untouched()
        # an open stepwise fit: refused, and the fit goes on
        Z, initial, _ = synth.make_synthetic(N, D, B, seed=3, sigma=6e-3, mix=0.5)
        ctx.set_samples(Z)
        sl = np.flatnonzero(initial == -1)[:100].astype(np.int64)
        ctx.fit_begin(B, initial, 5)
        refused(audit(), ESTATE, "stepwise")
        ctx.batch_begin(sl, 0, len(sl))
        for call in (audit, recruit, apairs, rpairs):
            refused(call(), ESTATE, "stepwise")
        guess = np.full(len(sl), -1, dtype=np.int64)
        ctx.batch_guess(guess)
        lab1 = np.full(len(sl), -9, dtype=np.int64)
        ctx.batch_round(guess, 0, lab1)
        ctx.batch_commit(lab1)
        assert np.array_equal(ctx.fit_labels()[sl], lab1) and np.all(lab1 >= 0)
        # chb_set_samples ends it, and the calls answer
        ctx.set_samples(X)
        assert audit() == 0 and np.all(obin >= 0) and np.isfinite(out["dist"][: 3 * B]).sum() > 0
        assert apairs() == 0 and rpairs() == 0 and np.all(oidx[3 * m:] == -77)
    finally:
        ctx.close()


# ---- 10. the context is left as found

def test_no_trace_left_in_a_fit():
    from chbin_amd import _lib, synth
    Nf, D, Bf, m, its = 1500, 72, 6, 5, 3
    Z, initial, _ = synth.make_synthetic(Nf + 100, D, Bf, seed=41, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:Nf]), np.ascontiguousarray(Z[Nf:])
    initial = initial[:Nf].copy()
    perms = synth.draw_permutations(initial, its, seed=0)

    def two_fits(wide_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(Bf, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in COUNTERS], ctx.fit_stats()))
                if k == 0 and wide_between:
                    assert ctx.counter("recruit_wide_rows") == 0
                    assert np.isfinite(ctx.audit_rows_wide(lab, Bf, 24)[2]).all()
                    assert np.isfinite(ctx.recruit_rows_wide(lab, Bf, 40, Y)[2]).all()
                    assert np.isfinite(ctx.audit_pairs_wide(lab, Bf, 64, np.arange(Nf), lab)).all()
                    assert ctx.counter("recruit_wide_rows") == 16384 and ctx.counter("pair_tiles") == tiles_of(lab, Bf)
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
