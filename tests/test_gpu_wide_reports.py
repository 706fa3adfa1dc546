"""chb_audit_rows_nearest_wide / chb_recruit_rows_nearest_wide / chb_bin_report_wide / chb_*_pairs_witness_wide: nearest
bins, bin report and pair witnesses for 16 < m <= 64, and the forwarding of m <= 16.

Yardsticks: each call is defined by the wide call that already exists (test_gpu_wide_m.py pins those to the oracle), so
almost everything here is BITWISE (uint64 views) against chb_audit_rows_wide / chb_recruit_rows_wide / chb_*_pairs_wide on
the same context: the ranking against the dense table (test_gpu_nearest_bins.check_against_dense), the report's tables
against test_gpu_bin_report.expected of the dense table and dsum against the header's block order computed in numpy,
the witness' dist / nbr_idx against the plain wide pair call and nbr_dist against chb_pairwise_distance.  The weights
have no bitwise yardstick: they are held to test_gpu_witness.py's rule -- feasible (>= 0, |sum - 1| < 1e-12, padding
exactly 0) and | ||alpha @ X[nbr] - y|| - dist | <= QP_TOL + 1e-7 scale (dist < 1e-6 scale) -- on the (D, m) cases on
which test_wide_m_cpu.py shows the oracle itself keeps feasibility 1e-12 and a duality gap below 1e-10 of the scale."""
import numpy as np
import pytest

import groups_reference  # noqa: F401  (the grouped calls' definition: labels with the row's group set to -1)
import row_reference  # noqa: F401
import wide_m_cases as W
from test_gpu_audit import QP_TOL
from test_gpu_bin_report import check_report, expected
from test_gpu_nearest_bins import check_against_dense
from test_gpu_pairs import COUNTERS, tiles_of
from test_gpu_witness import bits, check_padding, reconstruction_ratio, same

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
N, B, Q = W.N, W.B, W.Q
TWINS = 40
GROUPS = (np.arange(N, dtype=np.int64) // 4) * 1000 + 7   # four consecutive rows per group, ids neither dense nor small


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def ptr(a):
    return None if a is None else a.ctypes.data


def wide_rows(width, m):
    return min(16384, max(64, (256 << 20) // (width * (m + 1) * 4) // 64 * 64))


# ---- 1. nearest bins, bitwise against the dense wide call

@pytest.mark.parametrize("D", [21, 72])
@pytest.mark.parametrize("m", [17, 33, 64])
def test_nearest_bitwise(ctx, m, D):
    X, lab, Y, pairs = W.wide(D, twins=TWINS)
    ctx.set_samples(X)
    audit = ctx.audit_rows_wide(lab, B, m)
    grouped = ctx.audit_rows_wide(lab, B, m, groups=GROUPS)
    recruit = ctx.recruit_rows_wide(lab, B, m, Y)
    fin = np.isfinite(audit[1]).sum(axis=1)
    lone = int(np.flatnonzero(lab == 1)[0])
    assert np.all(audit[1][:, 0] == np.inf)              # the bin without a member
    assert fin[lone] == B - 2 and fin.max() == B - 1     # the lone member's row: one finite entry fewer than the others
    twin_rows = np.array([t for t, s in pairs])
    assert (np.sort(audit[1][twin_rows], axis=1)[:, 0] == 0.0).all()   # exact zeros: a twin sits on a vertex
    for k in (1, 3, 8, 16):
        got = ctx.audit_rows_nearest_wide(lab, B, m, k)
        check_against_dense(f"audit D={D} m={m} k={k}", got, audit, k)
        check_against_dense(f"grouped D={D} m={m} k={k}", ctx.audit_rows_nearest_wide(lab, B, m, k, groups=GROUPS), grouped, k)
        check_against_dense(f"recruit D={D} m={m} k={k}", ctx.recruit_rows_nearest_wide(lab, B, m, k, Y), recruit, k)
        if k >= 8:   # fewer finite entries than k: padded (k = 16 > B pads every row)
            assert np.all(got[0][:, B - 1:] == -1) and got[0][lone, B - 2] == -1 and got[0][lone, B - 3] >= 0
    assert not np.array_equal(bits(grouped[1]), bits(audit[1]))   # (the siblings were among the nearest members somewhere)
    # exact ties: a twin pair with two labels, offered as a new row, lies at distance 0 from both bins -- the lower bin
    # comes first
    tied = np.array([(t, s) for t, s in pairs if lab[t] != lab[s]])
    assert len(tied) > 10
    Yt = np.ascontiguousarray(X[tied[:, 0]])
    tb, td = ctx.recruit_rows_nearest_wide(lab, B, m, 3, Yt)
    check_against_dense(f"ties D={D} m={m}", (tb, td), ctx.recruit_rows_wide(lab, B, m, Yt), 3)
    assert np.all(td[:, :2] == 0.0) and np.all(td[:, 2] > 0.0)
    assert np.array_equal(tb[:, :2], np.sort(lab[tied], axis=1))
    nb, nd = ctx.audit_rows_nearest_wide(lab, B, m, 3)
    # a subset of rows with repeats keeps the caller's order
    rows = np.random.default_rng(51).integers(0, N, 300)
    sub = ctx.audit_rows_nearest_wide(lab, B, m, 3, rows)
    assert np.array_equal(sub[0], nb[rows]) and np.array_equal(bits(sub[1]), bits(nd[rows]))


def test_nearest_affine_metric(ctx):
    D, m, k = 72, 17, 3
    X, lab, Y, _ = W.wide(D, twins=TWINS)
    ctx.set_samples(X)
    convex = ctx.audit_rows_nearest_wide(lab, B, m, k)
    with ctx.using_metric("affine"):
        audit = ctx.audit_rows_wide(lab, B, m)
        recruit = ctx.recruit_rows_wide(lab, B, m, Y)
        got_a = ctx.audit_rows_nearest_wide(lab, B, m, k)
        got_r = ctx.recruit_rows_nearest_wide(lab, B, m, k, Y)
    check_against_dense("affine audit", got_a, audit, k)
    check_against_dense("affine recruit", got_r, recruit, k)
    assert not np.array_equal(bits(got_a[1]), bits(convex[1]))   # (the metric reached the kernel)


def test_nearest_across_the_chunk_edge(ctx):
    D, m, k = 21, 17, 3
    X, lab, Y, _ = W.wide(D, twins=TWINS)
    ctx.set_samples(X)
    reps = (16384 + 100 + Q - 1) // Q
    big = np.ascontiguousarray(np.tile(Y, (reps, 1))[:16384 + 100])
    dense = ctx.recruit_rows_wide(lab, B, m, big)
    assert ctx.counter("recruit_wide_rows") == wide_rows(B, m) == 16384 < len(big)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.recruit_rows_nearest_wide(lab, B, m, k, big)
    prof = {n: ctx.profile_get(n) for n in ("recruit_wide_select", "recruit_wide_solve", "nearest_bins", "recruit")}
    ctx.profile_enable(False)
    check_against_dense("two chunks", got, dense, k)
    for n in ("recruit_wide_select", "recruit_wide_solve", "nearest_bins"):
        assert prof[n]["launches"] == 2 and prof[n]["work"] == len(big) * B
    assert prof["recruit"]["launches"] == 0
    one = ctx.recruit_rows_nearest_wide(lab, B, m, k, Y)   # the rows behind the edge are the tiled rows again
    tail = (16384 + np.arange(100)) % Q
    assert np.array_equal(got[0][16384:], one[0][tail]) and np.array_equal(bits(got[1][16384:]), bits(one[1][tail]))


# ---- 2. bin report, bitwise

def block_order_dsum(own, dist, nb):
    """[nb, nb] of the header's summation order: a label's positions (in the caller's order) in blocks of 64, each block in
    order, the block sums in block order; labels and bins below nb only (the caller shows that the rest is empty)"""
    want = np.zeros((nb, nb))
    for a in range(nb):
        d = dist[own == a]
        for b in range(nb):
            total = 0.0
            for r0 in range(0, len(d), 64):
                s = 0.0
                for v in d[r0:r0 + 64, b]:
                    if np.isfinite(v):
                        s = s + float(v)
                total = total + s
            want[a, b] = total
    return want


def wild_labels(lab):
    """the labelling with a few rows labelled outside [0, B): they are members of no bin and are not scored"""
    out = lab.copy()
    out[np.random.default_rng(52).permutation(N)[:30]] = np.tile([-1, -7, B, B + 5, 1 << 40], 6)
    return out


@pytest.mark.parametrize("D", [21, 72])
@pytest.mark.parametrize("m", [17, 33, 64])
def test_bin_report_bitwise(ctx, m, D):
    X, lab, _, _ = W.wide(D, twins=TWINS)
    lab = wild_labels(lab)
    ctx.set_samples(X)
    for groups in (None, GROUPS):
        bins, dist, _, _ = ctx.audit_rows_wide(lab, B, m, groups=groups)
        got = ctx.bin_report_wide(lab, B, m, groups=groups)
        again = ctx.bin_report_wide(lab, B, m, groups=groups)
        check_report(f"D={D} m={m} groups={groups is not None}", got, expected(lab, B, None, bins, dist))
        assert got[5] == 30 and got[0].sum() + got[1].sum() + got[5] == N
        for a, b in zip(got, again):
            assert np.array_equal(a, b)
        assert np.array_equal(bits(got[4]), bits(again[4]))
        assert np.array_equal(bits(got[4]), bits(block_order_dsum(lab, dist, B)))


def test_bin_report_two_chunks(ctx):
    D, m = 21, 17
    X, lab, _, _ = W.wide(D, twins=TWINS)
    lab = wild_labels(lab)
    ctx.set_samples(X)
    rows = np.random.default_rng(53).integers(0, N, 20000)
    assert len(np.unique(rows)) < len(rows) and wide_rows(B, m) == 16384 < len(rows)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.bin_report_wide(lab, B, m, rows)
    prof = {n: ctx.profile_get(n) for n in ("audit_wide_select", "audit_wide_solve", "bin_report")}
    ctx.profile_enable(False)
    scored = int(np.count_nonzero((lab[rows] >= 0) & (lab[rows] < B)))
    for n in prof:
        assert prof[n]["launches"] == 2 and prof[n]["work"] == scored * B
    bins, dist, _, _ = ctx.audit_rows_wide(lab, B, m, rows)
    check_report("two chunks", got, expected(lab, B, rows, bins, dist))
    assert np.array_equal(bits(got[4]), bits(block_order_dsum(lab[rows], dist, B)))
    # the same positions in two calls, summed where sums are exact
    first, second = ctx.bin_report_wide(lab, B, m, rows[:9000]), ctx.bin_report_wide(lab, B, m, rows[9000:])
    for k in (0, 1, 2):
        assert np.array_equal(got[k], first[k] + second[k])
    assert np.array_equal(bits(got[3]), bits(np.minimum(first[3], second[3]))) and got[5] == first[5] + second[5]


def test_bin_report_short_chunks(ctx):
    """4096 bins (all but 8 empty) at m = 64: a dense wide chunk holds 192 rows, so the plan is cut there"""
    D, m, BB = 21, 64, 4096
    X, lab, _, _ = W.wide(D, twins=TWINS)
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows_wide(lab, BB, m)
    rows_per_chunk = ctx.counter("recruit_wide_rows")
    assert rows_per_chunk == wide_rows(BB, m) == 192 < N
    assert np.all(dist[:, B:] == np.inf) and np.all(bins < B)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.bin_report_wide(lab, BB, m)
    launches = ctx.profile_get("bin_report")["launches"]
    ctx.profile_enable(False)
    assert ctx.counter("recruit_wide_rows") == 192 and launches >= (N + 191) // 192
    small = expected(lab, B, None, bins, np.ascontiguousarray(dist[:, :B]))   # (the other 4088 bins have no member and no row)
    check_report("short chunks", tuple(a[:B, :B] if a.ndim == 2 else a[:B] for a in got[:5]) + (got[5],), small)
    assert np.array_equal(bits(got[4][:B, :B]), bits(block_order_dsum(lab, dist, B)))
    for k in (0, 2, 4):
        assert got[k].sum() == got[k][:B, :B].sum() and not got[k][B:].any() and not got[k][:, B:].any()
    assert not got[1][B:].any() and np.isinf(got[3][B:]).all() and np.isinf(got[3][:, B:]).all()


# ---- 3. witnesses

def shuffled_grid(n_rows, seed):
    """every (row, bin) pair, a fifth of them twice, shuffled"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(n_rows), np.arange(B), indexing="ij"), axis=-1).reshape(-1, 2)
    g = np.concatenate([g, g[rng.choice(len(g), len(g) // 5, replace=False)]])
    g = g[rng.permutation(len(g))]
    return np.ascontiguousarray(g[:, 0]), np.ascontiguousarray(g[:, 1])


def check_records(what, X, y, w, plain, pd_rows, m, convex=True):
    """w = (dist, idx, nd, alpha) of a witness call, plain = (dist, idx) of the plain wide pair call on the same pairs,
    pd_rows [P, n] = chb_pairwise_distance's rows of the scored rows"""
    dist, idx, nd, alpha = w
    assert idx.shape == nd.shape == alpha.shape == (len(dist), m) and idx.dtype == np.int64
    assert np.array_equal(bits(dist), bits(plain[0])), what
    assert np.array_equal(idx, plain[1]), what
    cnt = check_padding(idx, nd, alpha)
    assert np.array_equal(np.isinf(dist), cnt == 0) and cnt.max() == m and cnt.min() == 0
    real = idx >= 0
    want_nd = np.where(real, np.take_along_axis(pd_rows, np.where(real, idx, 0), axis=1), np.inf)
    assert np.array_equal(bits(nd), bits(want_nd)), what
    assert np.all(nd[:, 1:][real[:, 1:]] >= nd[:, :-1][real[:, 1:]])   # list order: by distance
    s = alpha.sum(axis=1)
    has = cnt > 0
    print(f"{what}: largest |sum - 1| = {np.abs(s[has] - 1.0).max():.3e}, smallest weight = {alpha.min():.3e}")
    assert np.all(np.abs(s[has] - 1.0) < 1e-12) and np.all(s[~has] == 0.0), what
    if convex:
        assert np.all(alpha >= 0.0), what
    ratio = reconstruction_ratio(X, y, dist, idx, nd, alpha)
    print(f"{what}: worst |reconstruction - dist| / bound over {len(ratio)} pairs = {ratio.max():.3e}")
    assert ratio.max() <= 1.0, what


def repeats_equal(w, key):
    _, first = np.unique(key, return_index=True)
    first_of = dict(zip(key[first].tolist(), first.tolist()))
    rep = np.array([first_of[k] for k in key.tolist()])
    assert len(first) < len(key) and same(w, tuple(a[rep] for a in w))


@pytest.mark.parametrize("D,m", [(72, 17), (72, 33), (72, 64), (21, 17)])
def test_witness(ctx, D, m):
    X, lab, Y, _ = W.wide(D, twins=TWINS)
    ctx.set_samples(X)
    pd = ctx.pairwise_distance()
    rows, pb = shuffled_grid(N, 54)
    for groups in (None, GROUPS):
        w = ctx.audit_pairs_witness_wide(lab, B, m, rows, pb, groups=groups)
        plain = ctx.audit_pairs_wide(lab, B, m, rows, pb, groups=groups, want_idx=True)
        check_records(f"audit D={D} m={m} groups={groups is not None}", X, X[rows], w, plain, pd[rows], m)
        repeats_equal(w, rows * B + pb)
        if groups is None:   # the lists are chb_topm_per_bin's
            assert np.array_equal(w[1], ctx.topm_per_bin(lab, B, m, np.arange(N))[0][rows, pb])
        else:                # no member of the row's group is a vertex
            real = w[1] >= 0
            assert not (GROUPS[np.where(real, w[1], 0)] == GROUPS[rows][:, None])[real].any()
    assert ctx.counter("pair_tiles") == tiles_of(pb, B)
    # new rows: the samples and the rows in one matrix (the rows unlabelled, members of no bin), so that
    # chb_pairwise_distance has the rows' distances to the samples
    XY = np.ascontiguousarray(np.vstack([X, Y]))
    lab2 = np.concatenate([lab, np.full(Q, -1, dtype=np.int64)])
    ctx.set_samples(XY)
    pd2 = ctx.pairwise_distance()
    row_of, rb = shuffled_grid(Q, 55)
    w = ctx.recruit_pairs_witness_wide(lab2, B, m, Y, row_of, rb)
    plain = ctx.recruit_pairs_wide(lab2, B, m, Y, row_of, rb, want_idx=True)
    check_records(f"recruit D={D} m={m}", XY, Y[row_of], w, plain, pd2[N + row_of], m)
    repeats_equal(w, row_of * B + rb)
    ctx.set_samples(X)   # (and on the samples alone the same records)
    assert same(w, ctx.recruit_pairs_witness_wide(lab, B, m, Y, row_of, rb))


def raw_audit(ctx, lab, groups, B_, m, rows, pb, P, dist, idx, nd, alpha):
    return ctx._lib.chb_audit_pairs_witness_wide(ctx._h, ptr(lab), ptr(groups), B_, m, ptr(rows), ptr(pb), P,
                                                 ptr(dist), ptr(idx), ptr(nd), ptr(alpha))


def raw_recruit(ctx, lab, B_, m, Y, Q_, D, row_of, pb, P, dist, idx, nd, alpha):
    return ctx._lib.chb_recruit_pairs_witness_wide(ctx._h, ptr(lab), B_, m, ptr(Y), Q_, D, ptr(row_of), ptr(pb), P,
                                                   ptr(dist), ptr(idx), ptr(nd), ptr(alpha))


def outputs(P, m, extra=5):
    """sentinel-filled outputs with room for `extra` pairs beyond P"""
    return (np.full(P + extra, -5.0), np.full((P + extra) * m, -55, dtype=np.int64), np.full((P + extra) * m, -5.0),
            np.full((P + extra) * m, -5.0))


def untouched(out, P, m):
    return all(np.all(a[(P if k == 0 else P * m):] == (-55 if a.dtype == np.int64 else -5.0)) for k, a in enumerate(out))


def test_witness_optional_outputs(ctx):
    D, m, P = 21, 33, 400
    X, lab, Y, _ = W.wide(D, twins=TWINS)
    lab = np.ascontiguousarray(lab)
    ctx.set_samples(X)
    rows, pb = (a[:P].copy() for a in shuffled_grid(N, 56))
    row_of, rb = (a[:P].copy() for a in shuffled_grid(Q, 57))
    full_a = tuple(a.reshape(-1) for a in ctx.audit_pairs_witness_wide(lab, B, m, rows, pb, groups=GROUPS))
    full_r = tuple(a.reshape(-1) for a in ctx.recruit_pairs_witness_wide(lab, B, m, Y, row_of, rb))
    for mask in range(1, 16):
        if (mask & 14) == 0:   # all three witness outputs null: refused (test_refusals_in_order)
            continue
        for full, call in ((full_a, lambda *o: raw_audit(ctx, lab, GROUPS, B, m, rows, pb, P, *o)),
                           (full_r, lambda *o: raw_recruit(ctx, lab, B, m, Y, Q, D, row_of, rb, P, *o))):
            out = outputs(P, m)
            assert call(*[o if mask >> k & 1 else None for k, o in enumerate(out)]) == 0, mask
            for k, o in enumerate(out):
                n = P if k == 0 else P * m
                if mask >> k & 1:
                    assert same((o[:n],), (full[k],)), (mask, k)
                else:
                    assert np.all(o == (-55 if o.dtype == np.int64 else -5.0))
            assert untouched(out, P, m)


def test_witness_affine_metric(ctx):
    D, m = 72, 17
    X, lab, _, _ = W.wide(D, twins=0)   # (independent vertices: 17 in 72 dimensions, no twins)
    ctx.set_samples(X)
    rows, pb = shuffled_grid(N, 58)
    with ctx.using_metric("affine"):
        dist, idx, nd, alpha = ctx.audit_pairs_witness_wide(lab, B, m, rows, pb)
        plain = ctx.audit_pairs_wide(lab, B, m, rows, pb, want_idx=True)
    assert np.array_equal(bits(dist), bits(plain[0])) and np.array_equal(idx, plain[1])
    cnt = check_padding(idx, nd, alpha)
    s = alpha.sum(axis=1)
    assert np.all(np.abs(s[cnt > 0] - 1.0) < 1e-12) and np.all(s[cnt == 0] == 0.0)
    assert (alpha < 0.0).any()   # (the affine hull's nearest point need not lie between the vertices)
    assert not np.array_equal(bits(dist), bits(ctx.audit_pairs_wide(lab, B, m, rows, pb)))


# ---- 4. m <= 16 forwards

@pytest.mark.parametrize("m", [5, 16])
def test_small_m_forwards(ctx, m):
    from chbin_amd import _lib
    lib = _lib.load()
    X, lab, Y, _ = W.wide(21, twins=TWINS)
    lab = np.ascontiguousarray(lab)
    ctx.set_samples(X)
    rng = np.random.default_rng(59)
    rows, pb, row_of = rng.integers(0, N, 300), rng.integers(0, B, 300), rng.integers(0, Q, 300)
    wide_before = ctx.counter("recruit_wide_rows")
    for g in (None, GROUPS):
        assert same(ctx.audit_rows_nearest_wide(lab, B, m, 3, rows, groups=g), ctx.audit_rows_nearest(lab, B, m, 3, rows, groups=g))
        assert same(ctx.bin_report_wide(lab, B, m, rows, groups=g)[:5], ctx.bin_report(lab, B, m, rows, groups=g)[:5])
        assert same(ctx.audit_pairs_witness_wide(lab, B, m, rows, pb, groups=g), ctx.audit_pairs_witness(lab, B, m, rows, pb, groups=g))
    assert same(ctx.recruit_rows_nearest_wide(lab, B, m, 3, Y), ctx.recruit_rows_nearest(lab, B, m, 3, Y))
    assert same(ctx.recruit_pairs_witness_wide(lab, B, m, Y, row_of, pb), ctx.recruit_pairs_witness(lab, B, m, Y, row_of, pb))
    assert ctx.counter("recruit_wide_rows") == wide_before

    # the refusals are the existing calls', code and text
    nb, nd = np.full(3 * 17, -55, dtype=np.int64), np.full(3 * 17, -5.0)
    three = np.array([3, 5, 699], dtype=np.int64)
    skipped = np.full(1, -55, dtype=np.int64)
    h = ctx._h

    def both(new, old):
        out = []
        for call in (new, old):
            rc = call()
            out.append((rc, lib.chb_last_error().decode()))
        assert out[0] == out[1] and out[0][0] < 0, out
        assert np.all(nb == -55) and np.all(nd == -5.0) and skipped[0] == -55
        return out[0]

    for k_, B_ in ((17, B), (3, 8193)):
        both(lambda: lib.chb_audit_rows_nearest_wide(h, ptr(lab), None, B_, m, k_, ptr(three), 3, ptr(nb), ptr(nd)),
             lambda: lib.chb_audit_rows_nearest(h, ptr(lab), None, B_, m, k_, ptr(three), 3, ptr(nb), ptr(nd)))
        both(lambda: lib.chb_recruit_rows_nearest_wide(h, ptr(lab), B_, m, k_, ptr(Y), 3, 21, ptr(nb), ptr(nd)),
             lambda: lib.chb_recruit_rows_nearest(h, ptr(lab), B_, m, k_, ptr(Y), 3, 21, ptr(nb), ptr(nd)))
    rc, text = both(lambda: lib.chb_audit_rows_nearest_wide(h, ptr(lab), None, B, m, 17, ptr(three), 3, ptr(nb), ptr(nd)),
                    lambda: lib.chb_audit_rows_nearest(h, ptr(lab), None, B, m, 17, ptr(three), 3, ptr(nb), ptr(nd)))
    assert rc == EUNSUPPORTED and "chb_audit_rows_nearest supports at most 16 nearest bins" in text
    both(lambda: lib.chb_audit_rows_nearest_wide(h, ptr(lab), None, B, m, 3, ptr(three), 3, None, None),
         lambda: lib.chb_audit_rows_nearest(h, ptr(lab), None, B, m, 3, ptr(three), 3, None, None))
    both(lambda: lib.chb_bin_report_wide(h, ptr(lab), None, 8193, m, ptr(three), 3, None, None, None, None, None, ptr(skipped)),
         lambda: lib.chb_bin_report(h, ptr(lab), 8193, m, ptr(three), 3, None, None, None, None, None, ptr(skipped)))
    both(lambda: lib.chb_bin_report_wide(h, ptr(lab), ptr(GROUPS), B, m, ptr(three), 3, None, None, None, None, None, None),
         lambda: lib.chb_bin_report_grouped(h, ptr(lab), ptr(GROUPS), B, m, ptr(three), 3, None, None, None, None, None, None))
    for B_, outs in ((8193, (ptr(nd), ptr(nb), None, None)), (B, (ptr(nd), None, None, None))):
        both(lambda: lib.chb_audit_pairs_witness_wide(h, ptr(lab), None, B_, m, ptr(three), ptr(three % B), 3, *outs),
             lambda: lib.chb_audit_pairs_witness(h, ptr(lab), None, B_, m, ptr(three), ptr(three % B), 3, *outs))
        both(lambda: lib.chb_recruit_pairs_witness_wide(h, ptr(lab), B_, m, ptr(Y), Q, 21, ptr(three % Q), ptr(three % B), 3, *outs),
             lambda: lib.chb_recruit_pairs_witness(h, ptr(lab), B_, m, ptr(Y), Q, 21, ptr(three % Q), ptr(three % B), 3, *outs))


# ---- 5. refusals in order, nothing written

def test_refusals_in_order():
    from chbin_amd import _lib, synth
    lib = _lib.load()
    D, m, k = 21, 17, 3
    X, lab, Y, _ = W.wide(D, twins=0)
    lab = np.ascontiguousarray(lab)
    ctx = _lib.Context(0)
    try:
        h = ctx._h
        rows = np.array([3, 5, 699], dtype=np.int64)
        pbins = np.array([1, 7, 4], dtype=np.int64)
        row_of = np.array([0, 199, 7], dtype=np.int64)
        f64 = {n: np.full(3 * 65 + 8, -77.0) for n in ("dist", "nd", "alpha", "near", "dmin", "dsum")}
        i64 = {n: np.full(3 * 65 + 8, -77, dtype=np.int64) for n in ("idx", "nbin", "conf", "unplaced", "dcnt", "skipped")}

        def nearest_a(B_=B, m_=m, k_=k, rows_=rows, Q_=3):
            return lib.chb_audit_rows_nearest_wide(h, ptr(lab), None, B_, m_, k_, ptr(rows_), Q_, ptr(i64["nbin"]), ptr(f64["near"]))

        def nearest_r(B_=B, m_=m, k_=k, D_=D, Q_=3):
            return lib.chb_recruit_rows_nearest_wide(h, ptr(lab), B_, m_, k_, ptr(Y), Q_, D_, ptr(i64["nbin"]), ptr(f64["near"]))

        def report(B_=B, m_=m, rows_=rows, Q_=3):   # (the small outputs only: a refused B = 8193 needs no B x B array)
            return lib.chb_bin_report_wide(h, ptr(lab), None, B_, m_, ptr(rows_), Q_, None, ptr(i64["unplaced"]), None, None, None,
                                           ptr(i64["skipped"]))

        def witness_a(B_=B, m_=m, rows_=rows, bins_=pbins, P_=3):
            return lib.chb_audit_pairs_witness_wide(h, ptr(lab), None, B_, m_, ptr(rows_), ptr(bins_), P_, ptr(f64["dist"]),
                                                    ptr(i64["idx"]), ptr(f64["nd"]), ptr(f64["alpha"]))

        def witness_r(B_=B, m_=m, D_=D, row_of_=row_of, bins_=pbins, P_=3):
            return lib.chb_recruit_pairs_witness_wide(h, ptr(lab), B_, m_, ptr(Y), Q, D_, ptr(row_of_), ptr(bins_), P_,
                                                      ptr(f64["dist"]), ptr(i64["idx"]), ptr(f64["nd"]), ptr(f64["alpha"]))

        calls = (nearest_a, nearest_r, report, witness_a, witness_r)

        def untouched():
            return all(np.all(a == -77.0) for a in f64.values()) and all(np.all(a == -77) for a in i64.values())

        def refused(rc, code, text=None):
            assert rc == code, (rc, lib.chb_last_error())
            if text:
                assert text in lib.chb_last_error().decode()
            assert untouched()

        # no samples: behind the ranges (k = 0 among them), before D, m, k and B
        for call in (nearest_a, nearest_r):
            refused(call(k_=0, m_=65, B_=8193), EINVAL, "k < 1")
        for call in calls:
            refused(call(m_=65, B_=8193), ESTATE)
        refused(nearest_r(D_=D + 1, k_=17), ESTATE)
        ctx.set_samples(X)
        # D before m; m = 65 before k = 17 before B = 8193; each on its own
        refused(nearest_r(D_=D + 1, m_=65), EINVAL)
        refused(witness_r(D_=D - 1, B_=8193), EINVAL)
        for call in calls:
            refused(call(m_=65, B_=8193), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(B_=8193), EUNSUPPORTED, "at most 8192 bins")
            refused(call(m_=0), EINVAL)
        for call in (nearest_a, nearest_r):
            refused(call(k_=0, m_=65), EINVAL, "k < 1")
            refused(call(k_=17, m_=65), EUNSUPPORTED, "at most 64 neighbours")
            refused(call(k_=17, B_=8193), EUNSUPPORTED, "at most 16 nearest bins")
        # every output null
        refused(lib.chb_audit_rows_nearest_wide(h, ptr(lab), None, B, m, k, ptr(rows), 3, None, None), EINVAL, "both null")
        refused(lib.chb_bin_report_wide(h, ptr(lab), None, B, m, ptr(rows), 3, None, None, None, None, None, None), EINVAL,
                "every output is null")
        refused(lib.chb_audit_pairs_witness_wide(h, ptr(lab), None, B, m, ptr(rows), ptr(pbins), 3, ptr(f64["dist"]), None, None,
                                                 None), EINVAL, "all null")
        refused(lib.chb_recruit_pairs_witness_wide(h, ptr(lab), B, m, ptr(Y), Q, D, ptr(row_of), ptr(pbins), 3, ptr(f64["dist"]),
                                                   None, None, None), EINVAL, "all null")
        # entries out of range
        bad = np.array([3, N, 5], dtype=np.int64)
        refused(nearest_a(rows_=bad), EINVAL, "row_idx")
        refused(witness_a(rows_=bad), EINVAL, "row_idx")
        refused(witness_a(bins_=np.array([1, B, 4], dtype=np.int64)), EINVAL, "bin_idx")
        refused(witness_r(row_of_=np.array([0, Q, 7], dtype=np.int64)), EINVAL, "row_of")
        i64["skipped"][0] = -77
        assert report(rows_=bad) == EINVAL and untouched()
        # nothing to score: no-ops that write nothing (the report: empty tables of a call without rows)
        tiles = ctx.counter("pair_tiles")
        for call in (nearest_a, nearest_r):
            assert call(Q_=0) == 0 and untouched()
        for call in (witness_a, witness_r):
            assert call(P_=0) == 0 and untouched()
        assert ctx.counter("pair_tiles") == tiles
        assert report(Q_=0) == 0 and i64["skipped"][0] == 0 and np.all(i64["unplaced"][:B] == 0) and np.all(i64["unplaced"][B:] == -77)
        i64["skipped"][0] = -77
        i64["unplaced"][:B] = -77
        # an open stepwise fit: refused, and the fit goes on
        Z, initial, _ = synth.make_synthetic(N, D, B, seed=3, sigma=6e-3, mix=0.5)
        ctx.set_samples(Z)
        sl = np.flatnonzero(initial == -1)[:100].astype(np.int64)
        ctx.fit_begin(B, initial, 5)
        refused(nearest_a(), ESTATE, "stepwise")
        ctx.batch_begin(sl, 0, len(sl))
        for call in calls:
            refused(call(), ESTATE, "stepwise")
        guess = np.full(len(sl), -1, dtype=np.int64)
        ctx.batch_guess(guess)
        lab1 = np.full(len(sl), -9, dtype=np.int64)
        ctx.batch_round(guess, 0, lab1)
        ctx.batch_commit(lab1)
        assert np.array_equal(ctx.fit_labels()[sl], lab1) and np.all(lab1 >= 0)
        # chb_set_samples ends it, and the calls answer within their bounds
        ctx.set_samples(X)
        for call in calls:
            assert call() == 0
        assert np.all(i64["nbin"][:3 * k] >= 0) and np.all(i64["nbin"][3 * k:] == -77) and np.all(f64["near"][3 * k:] == -77.0)
        assert np.all(i64["idx"][3 * m:] == -77) and np.all(f64["nd"][3 * m:] == -77.0) and np.all(f64["alpha"][3 * m:] == -77.0)
        assert np.all(f64["dist"][3:] == -77.0) and np.isfinite(f64["dist"][:3]).all()
        assert i64["skipped"][0] == 0 and np.all(i64["unplaced"][B:] == -77)
    finally:
        ctx.close()


# ---- 6. the context is left as found

def test_no_trace_left_in_a_fit():
    from chbin_amd import _lib, synth
    Nf, D, Bf, m, its = 1500, 72, 6, 5, 3
    Z, initial, _ = synth.make_synthetic(Nf + 100, D, Bf, seed=41, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:Nf]), np.ascontiguousarray(Z[Nf:])
    initial = initial[:Nf].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    groups = np.arange(Nf, dtype=np.int64) // 2
    ybins = np.arange(100, dtype=np.int64) % Bf

    def two_fits(calls_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(Bf, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in COUNTERS], ctx.fit_stats()))
                if k == 0 and calls_between:
                    assert ctx.counter("recruit_wide_rows") == 0 and ctx.counter("pair_tiles") == 0
                    before = ctx.audit_rows_wide(lab, Bf, 24)
                    assert (ctx.audit_rows_nearest_wide(lab, Bf, 24, 3)[0][:, 0] >= 0).all()
                    assert (ctx.recruit_rows_nearest_wide(lab, Bf, 40, 2, Y)[0][:, 0] >= 0).all()
                    assert sum(int(a.sum()) for a in ctx.bin_report_wide(lab, Bf, 33, groups=groups)[:2]) == Nf
                    assert ctx.counter("pair_tiles") == 0
                    assert np.isfinite(ctx.audit_pairs_witness_wide(lab, Bf, 64, np.arange(Nf), lab, groups=groups)[0]).all()
                    assert ctx.counter("pair_tiles") == tiles_of(lab, Bf)
                    assert np.isfinite(ctx.recruit_pairs_witness_wide(lab, Bf, 17, Y, np.arange(100), ybins)[0]).all()
                    assert ctx.counter("pair_tiles") == tiles_of(ybins, Bf) and ctx.counter("recruit_wide_rows") == 16384
                    assert [ctx.counter(n) for n in COUNTERS] == res[0][3]
                    assert ctx.fit_stats() == res[0][4]
                    assert np.array_equal(ctx.fit_labels(), lab)
                    after = ctx.audit_rows_wide(lab, Bf, 24)
                    assert same(before, after)
            return res
        finally:
            ctx.close()

    with_calls, without = two_fits(True), two_fits(False)
    for a, b in ((with_calls[0], with_calls[1]), (with_calls[1], without[1]), (with_calls[0], without[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert with_calls[1][3] == without[1][3] and with_calls[1][4] == without[1][4]


# ---- 7. the Python mirrors

def test_mirror_functions(ctx):
    from chbin_amd import _lib, clustering
    D, m, k = 72, 24, 3
    X, lab, Y, _ = W.wide(D, twins=TWINS)
    rows = np.arange(0, N, 3)
    nb = clustering.nearest_bins(X, lab, B, k=k, num_neighbors=m, rows=rows, groups=GROUPS)
    rnb = clustering.recruit_nearest_bins(X, lab, Y, B, k=k, num_neighbors=m)
    rep = clustering.bin_report(X, lab, B, num_neighbors=m, groups=GROUPS)
    assert isinstance(nb, clustering.NearestBins) and isinstance(rnb, clustering.NearestBins) and isinstance(rep, clustering.BinReport)
    pos, pbins = nb.pairs()   # the two nearest bins of every row, into the witness call at the same m
    assert len(pos) > len(rows)
    wit = clustering.witness(X, lab, rows[pos], pbins, B, num_neighbors=m, groups=GROUPS)
    ypos, ybins = rnb.pairs(ranks=(0,))
    rwit = clustering.recruit_witness(X, lab, Y, ypos, ybins, B, num_neighbors=m)
    assert isinstance(wit, clustering.Witness) and wit.neighbors.shape == (len(pos), m)
    assert _lib.default_context().get_metric() == "convex"
    ctx.set_samples(X)
    assert same((nb.bins, nb.dist), ctx.audit_rows_nearest_wide(lab, B, m, k, rows, groups=GROUPS))
    assert same((rnb.bins, rnb.dist), ctx.recruit_rows_nearest_wide(lab, B, m, k, Y))
    assert same((rep.confusion, rep.unplaced, rep.dcnt, rep.dmin, rep.dsum), ctx.bin_report_wide(lab, B, m, groups=GROUPS)[:5])
    assert same((wit.dist, wit.neighbors, wit.neighbor_dist, wit.weights),
                ctx.audit_pairs_witness_wide(lab, B, m, rows[pos], pbins, groups=GROUPS))
    assert same((rwit.dist, rwit.neighbors, rwit.neighbor_dist, rwit.weights),
                ctx.recruit_pairs_witness_wide(lab, B, m, Y, ypos, ybins))
    # end to end: the witness' distance is the ranked one, and the nearest point lies at it
    assert np.array_equal(bits(wit.dist), bits(nb.dist[:, :2][nb.bins[:, :2] >= 0]))
    assert np.array_equal(bits(rwit.dist), bits(rnb.dist[ypos, 0]))
    real = wit.neighbors >= 0
    has = wit.count > 0
    assert has.all() and np.array_equal(wit.count, real.sum(axis=1))
    blocks = [(0, 10), (10, D - 3), (D - 3, D)]   # a partition of the columns
    res = wit.residual_by_block(X, X[rows[pos]], blocks)
    assert res.shape == (len(pos), 3) and np.all(res >= 0.0)
    # the blocks' sum is dist**2 within the witness bound in squared form: |r^2 - d^2| = |r - d| (r + d) <= b (2 d + b)
    scale = np.where(real, wit.neighbor_dist, 0.0).max(axis=1)
    d = wit.dist
    b = QP_TOL + 1e-7 * scale * (d < 1e-6 * scale)
    assert np.all(np.abs(res.sum(axis=1) - d ** 2) <= b * (2.0 * d + b))
    with pytest.raises(_lib.ChbError, match="at most 64 neighbours"):
        clustering.nearest_bins(X, lab, B, k=k, num_neighbors=65)
