"""Wide row scoring (16 < m <= 64: recruit_select_wide_kernel, hull_wide_kernel<32 | 64>, the Wave64T backend on the
un-normalised Gram) on the data test_gpu_wide_m.py does not offer it: ill-scaled, tied and of odd feature widths.  The
cases are wide_scale_cases.py's, the yardstick hull_certificate.py's bracket [lo, hi], which contains the true distance
whatever solver found it and which test_hull_certificate_cpu.py shows to be narrower than 1e-10 of the scale on every
problem used here -- so exactly dependent vertex sets (duplicates, one-hot rows, 64 vertices in 1 to 33 dimensions) have
a yardstick that shares nothing with the driver under test.

Per kind and m, for audit_rows_wide and recruit_rows_wide: no NaN, the +inf pattern exactly, every finite entry in
[lo - bound, hi + bound] with bound = row_reference.bound (1e-9 of the scale, and 1e-7 of it more below 1e-6 of the
scale -- the family's envelope, not a new number); the bin equal to the reference's on every clear row (at most 1 % of a
case's rows are not: proven there; where ties are the construction the chosen bin's reference distance is within the bound
of the reference minimum instead); bin, min_dist and margin bitwise the strict scan of the call's own table.  Exact zeros
for `identical` and `onehot`.  The lists of audit_pairs_wide / recruit_pairs_wide over the whole grid equal the
reference's index sets, padding included, and topm_per_bin's; their distances are bitwise the dense entries (the grid is
scored shuffled, every bin's last tile is short).  The same per feature width.  The affine metric on `offset`, `tiny` and
`huge` against the lstsq reference within the same bound.

What a wrong kernel would trip.  A slab shift that loses the hand-over from lane 15 of slab r - 1 to lane 0 of slab r
drops an entry whenever a later member tile offers a nearer member to a list of more than 16: every index-set comparison
here fails, and on `identical` / `onehot` the failing lists are single runs of equal distances, where only the sample
index orders entries 15/16, 31/32 and 47/48.  A tie rule that looks at the distance alone reorders or mis-cuts those runs.
A solver threshold that is absolute instead of relative to the lifted norm rejects every vertex on `tiny` (a Gram of
1e-104-sized entries) and leaves the bracket by the distance between nearest vertex and hull.  A feature loop that assumes
a second step, or a prefetch on every full step, shows at D <= 16 and at padded widths that are multiples of 16, which no
other test of the wide kernels runs.  (Testing a lane quarter's range against D instead of the padded width is NOT a
defect: the padding is zero, and a quarter with one real feature passes either test.)  A driver defect on duplicated or
low-rank vertex sets no longer hides behind chb_hull_distance_batch, the same driver.

Largest |d - mid| / scale seen on an MI355X (recruit and audit, every m of the case), entries with a reference above
1e-6 of the scale:
  offset 1.4e-15   tiny 1.6e-15   huge 1.3e-15   wide 1.6e-14 (m = 64; 4.1e-15 at m = 17)   outlier 1.5e-15
  spread 1.1e-15   identical 1.2e-15   onehot 0   affine metric 2.0e-15
  D = 1: 0   2: 7.7e-15   7: 5.7e-13 (the bracket's own width there is 1.1e-12)   8: 2.1e-14   9: 1.6e-14
  D = 16, 17, 32, 33, 136, 300, 600: at most 4.4e-15
and below 1e-6 of the scale (rows inside a hull of 17 to 64 members in 1 to 9 dimensions; the bound allows 1e-7 there,
the root of a rounding-sized square): at most 5.3e-9.  Rounding-sized everywhere: no defect of the wide kernels, of the
Wave64T backend or of the driver was found, and the un-normalised Gram holds at 1e-50 and 1e+50.  The bound is not tuned
to these figures."""
import numpy as np
import pytest

import hull_certificate as H
import wide_scale_cases as C
from row_reference import RowReference, bound, clear_rows
from test_gpu_pairs import bits
from test_gpu_recruit import strict_scan

pytestmark = pytest.mark.gpu

B = C.B


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check_table(what, got, cert, exempt):
    """A dense call's (bins, dist, min_dist, margin) against the bracket; returns the largest |d - mid| / scale"""
    bins, dist, mind, margin = got
    fin = np.isfinite(cert.hi)
    assert dist.shape == cert.hi.shape, what
    assert not np.isnan(dist).any(), what
    assert np.array_equal(np.isfinite(dist), fin), what
    assert np.all(dist[~fin] == np.inf), what   # (+inf, not -inf)
    ref = H.as_reference(cert)
    bnd = bound(ref)
    pos = fin & (cert.scale > 0.0)
    with np.errstate(invalid="ignore"):
        rel = np.where(pos, np.abs(dist - ref.dist) / np.where(pos, cert.scale, 1.0), 0.0)
        zeroish = pos & (ref.dist < 1e-6 * cert.scale)   # (where the bound allows the root of a rounding-sized square)
    worst, worst0 = rel[pos & ~zeroish].max(initial=0.0), rel[zeroish].max(initial=0.0)
    print(f"{what}: worst |d - mid| / scale = {worst:.3e} over {int((pos & ~zeroish).sum())} entries, "
          f"{worst0:.3e} over {int(zeroish.sum())} with a reference below 1e-6 of the scale")
    low, high = dist[fin] < (cert.lo - bnd)[fin], dist[fin] > (cert.hi + bnd)[fin]
    assert not low.any() and not high.any(), (what, int(low.sum()), int(high.sum()), worst)
    # the reduction: bitwise the strict scan of the call's own table
    b2, d2, g2 = strict_scan(dist)
    assert np.array_equal(bins, b2), what
    assert np.array_equal(bits(mind), bits(d2)) and np.array_equal(bits(margin), bits(g2)), what
    best, clear = clear_rows(ref)
    if exempt:
        q = np.arange(len(bins))
        assert np.all(bins >= 0), what
        gap = ref.dist[q, bins] - ref.dist.min(axis=1)
        assert np.all(gap <= bnd[q, bins]), (what, gap.max())
    else:
        n_out = int(np.count_nonzero(~clear))
        assert n_out <= 0.01 * len(bins), (what, n_out)
        assert np.array_equal(bins[clear], best[clear]), what
    return worst


def check_lists(what, ctx, labels, m, Y, audit_sets, recruit_sets, dense_audit, dense_recruit):
    """The pair calls over the whole grid, scored shuffled: index sets against the reference's and topm_per_bin's,
    distances bitwise against the dense tables"""
    N, Q = len(audit_sets), len(recruit_sets)
    order = np.random.default_rng(31).permutation(N * B)
    dist, idx = ctx.audit_pairs_wide(labels, B, m, order // B, order % B, want_idx=True)
    back = np.argsort(order)
    assert idx.dtype == np.int64 and idx.shape == (N * B, m), what
    idx, dist = idx[back].reshape(N, B, m), dist[back].reshape(N, B)
    want = H.padded(audit_sets, B, m)
    assert np.array_equal(idx, want), (what, "audit", int((idx != want).any(axis=2).sum()))
    tidx, _, cnt = ctx.topm_per_bin(labels, B, m, np.arange(N))
    assert np.array_equal(idx, tidx) and np.array_equal((idx >= 0).sum(axis=2), cnt), what
    assert np.array_equal(bits(dist), bits(dense_audit)), (what, "audit pairs against dense")
    order = np.random.default_rng(32).permutation(Q * B)
    dist, idx = ctx.recruit_pairs_wide(labels, B, m, Y, order // B, order % B, want_idx=True)
    back = np.argsort(order)
    idx, dist = idx[back].reshape(Q, B, m), dist[back].reshape(Q, B)
    want = H.padded(recruit_sets, B, m)
    assert np.array_equal(idx, want), (what, "recruit", int((idx != want).any(axis=2).sum()))
    assert np.array_equal(bits(dist), bits(dense_recruit)), (what, "recruit pairs against dense")
    assert N % 64 != 0 and Q % 64 != 0   # (every bin's last tile is short)


# ---- 1. distances on ill-scaled and tied data

@pytest.mark.parametrize("m", C.MS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_distances_lie_in_the_bracket(ctx, kind, m):
    X, labels, Y, rows, copies = C.case_data(kind)
    ctx.set_samples(X)
    got = {"recruit": ctx.recruit_rows_wide(labels, B, m, Y), "audit": ctx.audit_rows_wide(labels, B, m, rows)}
    for call, res in got.items():
        cert = C.case_certificate(kind, call, m)
        check_table(f"{kind} m={m} {call}", res, cert, kind in C.EXEMPT)
        dist = res[1]
        if kind == "identical":
            # a copy of a labelled member has that member as a candidate -- in the audit too, where only the row itself
            # is withheld and its twins stay: exactly 0
            mine = copies[0] if call == "recruit" else copies[1]
            assert len(mine) >= 10 and np.all(dist[mine, 0] == 0.0), (kind, m, call)
        if kind == "onehot":
            zero = cert.hi == 0.0
            assert zero.any() and np.array_equal(dist == 0.0, zero), (kind, m, call)
            n = np.array([1.0, 2.0])
            off = np.abs(dist[~zero][:, None] - np.sqrt(1.0 + 1.0 / n)[None, :]).min(axis=1)
            assert np.all(off <= 1e-9 * cert.scale[~zero]), (kind, m, call, off.max())


# ---- 2. selection under ties, and the pair calls against the dense ones

@pytest.mark.parametrize("m", C.MS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_lists_are_the_reference_sets_and_pairs_equal_dense(ctx, kind, m):
    X, labels, Y, _, _ = C.case_data(kind)
    ctx.set_samples(X)
    audit_sets, recruit_sets = C.grid_sets(kind)
    check_lists(f"{kind} m={m}", ctx, labels, m, Y, audit_sets, recruit_sets,
                ctx.audit_rows_wide(labels, B, m)[1], ctx.recruit_rows_wide(labels, B, m, Y)[1])


# ---- 3. the feature width

@pytest.mark.parametrize("m", C.WMS)
@pytest.mark.parametrize("D", C.WIDTHS)
def test_feature_widths(ctx, D, m):
    X, lab, Y, rows = C.width_data(D)
    ctx.set_samples(X)
    audit = ctx.audit_rows_wide(lab, B, m)
    recruit = ctx.recruit_rows_wide(lab, B, m, Y)
    check_table(f"D={D} m={m} audit", [a[rows] for a in audit], C.width_certificate(D, "audit", m), D in C.WEXEMPT)
    check_table(f"D={D} m={m} recruit", recruit, C.width_certificate(D, "recruit", m), D in C.WEXEMPT)
    assert np.all(audit[1][:, 0] == np.inf)   # the bin without a member
    if D == 1:
        cert = C.width_certificate(D, "recruit", m)
        want = np.array([[C.closed_form_1d(Y[q, 0], X[cert.sets[q][c], 0]) for c in range(1, B)] for q in range(len(Y))])
        ref = RowReference(want, cert.scale[:, 1:], None)
        assert np.all(np.abs(recruit[1][:, 1:] - want) <= bound(ref)), (D, m)
    audit_sets, recruit_sets = C.width_grid_sets(D)
    check_lists(f"D={D} m={m}", ctx, lab, m, Y, audit_sets, recruit_sets, audit[1], recruit[1])


# ---- 4. the affine metric

@pytest.mark.parametrize("m", [17, 64])
@pytest.mark.parametrize("kind", ["offset", "tiny", "huge"])
def test_affine_metric(ctx, kind, m):
    X, labels, Y, rows, _ = C.case_data(kind)
    assert m <= 64 < X.shape[1]   # (generic rows: every selected set is affinely independent)
    ctx.set_samples(X)
    with ctx.using_metric("affine"):
        got = {"recruit": ctx.recruit_rows_wide(labels, B, m, Y)[1], "audit": ctx.audit_rows_wide(labels, B, m, rows)[1]}
    for call, dist in got.items():
        cert = C.case_certificate(kind, call, m)   # (the sets and the scales: the selection knows no metric)
        src = Y if call == "recruit" else X[rows]
        want = np.array([[H.affine_distance(X[s] - src[q]) for s in per_bin] for q, per_bin in enumerate(cert.sets)])
        ref = RowReference(want, cert.scale, None)
        assert np.isfinite(dist).all() and dist.shape == want.shape
        assert np.all(want <= cert.hi + 1e-12 * cert.scale)   # (the affine hull contains the hull)
        err = np.abs(dist - want)
        print(f"{kind} m={m} {call} affine: worst |d - ref| / scale = {(err / cert.scale).max():.3e}")
        assert np.all(err <= bound(ref)), (kind, m, call)
