"""Row scoring (recruit_kernel<kResident, kMulti, kPairs>, its reduce and bin_report_kernel) on ill-scaled data, against
the shift-invariant reference of row_reference.py.

The other GPU tests of this family run on the generator's friendly data (values in [0, 1], sigma 6e-3 .. 8e-3) and hold
the kernels against oracle.sweep, which is unfit on anything else.  Here the data carries a large offset, a scale of 1e-50
or 1e+50, wildly different column scales, one huge outlier, bins far apart, 150 equal members on the selection edge, or
nothing but exact ties (one-hot rows), and every distance is held against reference_rows: the oracle's selection, then the
enumerator (up to 12 vertices) or Goldfarb-Idnani (13 to 16) on the problem shifted to the row.

Per case, for recruit_rows and audit_rows: the +inf pattern exactly, no NaN, no -inf; finite entries within
1e-9 * scale + 1e-7 * scale * (ref < 1e-6 * scale), scale = max_i ||p_i - x|| -- the relative envelope of
test_hull_distance_16_lane_solver_both_starts, not a new number; the bin equal to the reference's on every row whose
reference margin exceeds twice the bound of its two best entries (at most 1 % of a case's rows may be left out by that
rule: test_row_reference_cpu.py proves it from the reference alone; `identical` and `onehot`, where ties are the
construction, check instead that the chosen bin's reference distance is within the bound of the reference minimum); bin,
min_dist and margin exactly the strict scan over the call's own distances.  Then: exact zeros (`identical`, `onehot`),
topm_per_bin's index sets against the reference's, the list calls and the pair calls bit for bit against the dense calls,
and bin_report against the audit of the same call.

Largest |d - ref| / scale seen on an MI355X, per kind (recruit and audit, every m and D of the kind):
  offset 7.4e-16 (D = 300)   tiny 5.4e-16   huge 4.7e-16   wide 3.2e-15 (m = 16; 4.2e-16 at m <= 12)
  outlier 6.9e-16            spread 5.0e-16  identical 6.4e-16   onehot 0
i.e. rounding-sized at every kind: no defect of the family was found here.  The m = 1 slice of a list call equals the
nearest member's k-sequential distance bit for bit on about two thirds of the entries and is within 2 ulp of it on the rest (the
Gram diagonal is summed in the matrix core's order): see test_list_calls_equal_the_single_calls."""
import functools

import numpy as np
import pytest

from row_reference import bound, clear_rows, reference_rows
from test_gpu_bin_distances import TINY
from test_gpu_bin_report import check_report, expected
from test_gpu_neighbor_sweep import check_slices
from test_gpu_recruit import check_reduction, strict_scan

pytestmark = pytest.mark.gpu

N = 600
KINDS = ("offset", "tiny", "huge", "wide", "outlier", "spread", "identical", "onehot")
EXEMPT = ("identical", "onehot")   # ties are the construction: no cap, another bin check
HUGE = 1e+50                       # (squares of 1e+50-sized entries stay far inside fp64)
N_EQUAL, N_COPIES = 150, 10        # `identical`: equal members of bin 0; copies of them among the scored rows
MS = (1, 2, 5, 12)

# name: kind, D, B, m, Q (new rows: 130 = three 64-row tiles with a last tile of 2; 66 = two, the last of 2); rseed draws
# the labels and the deformation, chosen per case so that the cap holds by the reference alone
CASES = {}
for _k in KINDS:
    CASES[f"{_k}_m5"] = dict(kind=_k, D=24 if _k == "onehot" else 136, B=4, m=5, Q=130)
for _k in KINDS:   # the enumerator's limit; the multi-step active set of solve16
    CASES[f"{_k}_m12"] = dict(kind=_k, D=24 if _k == "onehot" else 136, B=3, m=12, Q=66)
for _k in ("identical", "wide"):
    CASES[f"{_k}_m16"] = dict(kind=_k, D=136, B=4, m=16, Q=130)
CASES["offset_d300"] = dict(kind="offset", D=300, B=4, m=5, Q=130)
NAMES = list(CASES)
MULTI_KINDS = ("tiny", "huge", "wide", "identical")
REPORT_KINDS = ("tiny", "huge", "spread")


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, labels, Y, rows, copies) of a case; deterministic.  One generator draw of N + Q rows, deformed as a whole and
    then cut into the resident rows X and the new rows Y; labels = the true labels of X with about 30 % set to -1; rows =
    the audited rows, every third resident row; copies = None, or for `identical` (positions in Y, positions in rows) of
    the scored rows that are copies of the equal members."""
    from chbin_amd import synth
    c = CASES[name]
    kind, D, B, m, Q = c["kind"], c["D"], c["B"], c["m"], c["Q"]
    rng = np.random.default_rng(c.get("rseed", 7))
    if kind == "onehot":
        # test_gpu_fused_trim.case_data's: bin c owns the columns 2 c and 2 c + 1; a row is at distance 0 from copies of
        # itself and at exactly sqrt(2) from every other row
        i = np.arange(N + Q)
        true = i % B
        Z = np.zeros((N + Q, D))
        Z[i, 2 * true + (i // B) % 2] = 1.0
    else:
        Z, _, true = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    labels = true[:N].copy()
    labels[rng.random(N) < 0.3] = -1
    rows = np.arange(0, N, 3, dtype=np.int64)
    copies = None
    if kind == "offset":
        Z = Z + 1000.0
    elif kind == "tiny":
        Z = Z * TINY
    elif kind == "huge":
        Z = Z * HUGE
    elif kind == "wide":
        Z = Z * rng.lognormal(0, 3, size=(1, D))
    elif kind == "outlier":
        member = np.flatnonzero((labels >= 0) & (np.arange(N) % 3 == 0))[5]   # (a labelled member that is audited)
        Z[member, 3] = 1e6
        Z[N + 7, 3] = 1e6
    elif kind == "spread":
        Z = Z + 1e3 * true[:, None] * rng.random((1, D))
    elif kind == "identical":
        # 150 labelled rows, scattered over the sample indices, become equal members of bin 0: more than two 64-row member
        # tiles and more than m, so the tie sits on the selection edge across tiles
        ids = rng.choice(np.flatnonzero(labels >= 0), N_EQUAL, replace=False)
        labels[ids] = 0
        Z[ids] = Z[ids[0]]
        ycopies = np.sort(rng.choice(Q, N_COPIES, replace=False))
        Z[N + ycopies] = Z[ids[0]]
        copies = (ycopies, np.flatnonzero(np.isin(rows, ids)))
        assert len(copies[1]) >= N_COPIES
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    for a in (X, labels, Y, rows):
        a.setflags(write=False)
    return X, labels, Y, rows, copies


@functools.lru_cache(maxsize=None)
def case_reference(name, call, m=None):
    """reference_rows of a case's recruit or audit call (with the index sets), at the case's m or another"""
    c = CASES[name]
    X, labels, Y, rows, _ = case_data(name)
    m = c["m"] if m is None else m
    if call == "recruit":
        return reference_rows(X, labels, c["B"], m, Y=Y, want_sets=True)
    return reference_rows(X, labels, c["B"], m, rows=rows, want_sets=True)


def left_out(name, call):
    """(rows the tie rule leaves out, rows) of a case's call, by the reference alone"""
    _, clear = clear_rows(case_reference(name, call))
    return int(np.count_nonzero(~clear)), len(clear)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check_against_reference(name, call, bins, dist, ref):
    kind = CASES[name]["kind"]
    fin = np.isfinite(ref.dist)
    assert not np.isnan(dist).any(), (name, call)
    assert np.array_equal(np.isfinite(dist), fin), (name, call)
    assert np.all(dist[~fin] == np.inf), (name, call)   # (+inf, not -inf)
    err = np.abs(dist - ref.dist)[fin]
    scale = ref.scale[fin]
    pos = scale > 0.0
    worst = (err[pos] / scale[pos]).max() if pos.any() else 0.0
    print(f"{name} {call}: worst |d - ref| / scale = {worst:.3e} over {int(fin.sum())} finite entries")
    over = err > bound(ref)[fin]
    assert not over.any(), (name, call, f"{int(over.sum())} of {err.size} entries off, worst {worst:.3e} of the scale")
    best, clear = clear_rows(ref)
    assert np.array_equal(best, strict_scan(ref.dist)[0])   # (the reference's bin is the strict scan's)
    if kind in EXEMPT:
        q = np.arange(len(bins))
        assert np.all(bins >= 0), (name, call)
        gap = ref.dist[q, bins] - ref.dist.min(axis=1)
        assert np.all(gap <= bound(ref)[q, bins]), (name, call, gap.max())
    else:
        n_out = int(np.count_nonzero(~clear))
        print(f"{name} {call}: {n_out} of {len(bins)} rows within twice the bound of a tie")
        assert n_out <= 0.01 * len(bins), (name, call, n_out)
        assert np.array_equal(bins[clear], best[clear]), (name, call)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_recruit_and_audit_match_the_reference(ctx, name):
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, Y, rows, copies = case_data(name)
    ctx.set_samples(X)
    got = {"recruit": ctx.recruit_rows(labels, B, m, Y), "audit": ctx.audit_rows(labels, B, m, rows)}
    for call, (bins, dist, mind, margin) in got.items():
        ref = case_reference(name, call)
        assert dist.shape == ref.dist.shape
        check_reduction(bins, dist, mind, margin)
        check_against_reference(name, call, bins, dist, ref)
        if c["kind"] == "identical":
            # a copy of a labelled member has that member as a candidate -- in the audit too, where only the row itself is
            # withheld and its twins stay: exactly 0
            mine = copies[0] if call == "recruit" else copies[1]
            assert len(mine) >= N_COPIES and np.all(dist[mine, 0] == 0.0), (name, call)
        if c["kind"] == "onehot":
            # hulls of orthogonal unit vectors: 0, or sqrt(1 + 1 / n) with n = the distinct points (of the bin's two) selected
            zero = ref.dist == 0.0
            assert zero.any() and np.array_equal(dist == 0.0, zero), (name, call)
            n = np.array([1.0, 2.0])
            assert np.all(np.abs(ref.dist[~zero][:, None] - np.sqrt(1.0 + 1.0 / n)[None, :]).min(axis=1) < 1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_topm_per_bin_returns_the_reference_sets(ctx, name):
    """The list route's selection on the same context and labels: the reference's sets are the ones both routes use."""
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, _, rows, _ = case_data(name)
    sets = case_reference(name, "audit").sets
    ctx.set_samples(X)
    pick = np.arange(0, len(rows), len(rows) // 40)[:40]
    idx, _, cnt = ctx.topm_per_bin(labels, B, m, rows[pick])
    for k, q in enumerate(pick):
        for b in range(B):
            want = sets[q][b]
            assert cnt[k, b] == len(want), (name, q, b)
            assert np.array_equal(idx[k, b, :len(want)], want), (name, q, b)


@pytest.mark.parametrize("kind", MULTI_KINDS)
def test_list_calls_equal_the_single_calls(ctx, kind):
    name = f"{kind}_m5"
    B = CASES[name]["B"]
    X, labels, Y, rows, _ = case_data(name)
    ctx.set_samples(X)
    multi = {"recruit": ctx.recruit_rows_multi(labels, B, MS, Y), "audit": ctx.audit_rows_multi(labels, B, MS, rows)}
    check_slices(multi["recruit"], [ctx.recruit_rows(labels, B, m, Y) for m in MS])
    check_slices(multi["audit"], [ctx.audit_rows(labels, B, m, rows) for m in MS])
    # m = 1: the hull is the nearest member and the distance its distance, sqrt(sum_k y_k^2) with y = p - x.  The
    # selection sums the squares k-sequentially and unfused (chb_pairwise_distance's arithmetic, which the reference's
    # cdist_row restates); the returned distance is the diagonal of the matrix-core Gram tile of the same y, summed in the
    # matrix core's order.  Where cdist_row's sum agrees in every order -- at most one y_k is not zero, so no sum rounds --
    # the two are equal bit for bit.  Elsewhere each is a sum of D non-negative squares of the SAME y_k (one IEEE
    # subtraction each), off by at most (D + 1) u of the exact sum whatever the order and the fusing (u = 2^-53), so the
    # two sums differ by at most 2 (D + 1) u, their roots by half of that and a rounding each: (D + 3) u of the distance.
    from oracle import oracle as O
    D = X.shape[1]
    for call, (_, dist, _, _) in multi.items():
        ref = case_reference(name, call, 1)
        src = Y if call == "recruit" else X[rows]
        near = np.full(ref.dist.shape, np.inf)
        exact = np.zeros(ref.dist.shape, dtype=bool)
        for q in range(len(src)):
            for b in range(B):
                if len(ref.sets[q][b]):
                    p = X[ref.sets[q][b][0]]
                    near[q, b] = O.cdist_row(np.vstack([src[q], p]), 0)[1]
                    exact[q, b] = np.count_nonzero(p - src[q]) <= 1
        assert np.isfinite(near).all()   # (no bin of these cases is empty)
        assert np.array_equal(bits(near), bits(ref.dist)), (name, call)   # (the enumerator's one-vertex value is that sum)
        d1 = dist[MS.index(1)]
        same = bits(d1) == bits(near)
        ulp = np.abs(d1 - near)[~exact] / np.spacing(near[~exact])
        print(f"{name} {call}: m = 1 slice bit for bit the nearest member's distance on {int(same.sum())} of {same.size} "
              f"entries ({int(exact.sum())} of them exact in every order), at most {ulp.max():.0f} ulp off")
        assert np.all(same[exact]), (name, call)
        assert np.all(np.abs(d1 - near) <= (D + 3) * 2.0 ** -53 * near), (name, call, ulp.max())
        if kind == "identical":
            assert exact.sum() >= N_COPIES


@pytest.mark.parametrize("kind", MULTI_KINDS)
def test_pair_calls_equal_the_dense_entries(ctx, kind):
    name = f"{kind}_m5"
    c = CASES[name]
    B, m, Q = c["B"], c["m"], c["Q"]
    X, labels, Y, rows, _ = case_data(name)
    rng = np.random.default_rng(31)
    ctx.set_samples(X)
    _, dense, _, _ = ctx.recruit_rows(labels, B, m, Y)
    # 200 random pairs and every row against bin 1: tiles of 64 and a short tail
    row_of = np.concatenate([rng.integers(0, Q, 200), np.arange(Q)])
    pb = np.concatenate([rng.integers(0, B, 200), np.full(Q, 1)])
    got = ctx.recruit_pairs(labels, B, m, Y, row_of, pb)
    assert np.array_equal(bits(got), bits(dense[row_of, pb])), name
    _, dense, _, _ = ctx.audit_rows(labels, B, m, rows)
    pos = np.concatenate([rng.integers(0, len(rows), 200), np.arange(len(rows))])
    pb = np.concatenate([rng.integers(0, B, 200), np.full(len(rows), 1)])
    got = ctx.audit_pairs(labels, B, m, rows[pos], pb)
    assert np.array_equal(bits(got), bits(dense[pos, pb])), name


@pytest.mark.parametrize("kind", REPORT_KINDS)
def test_bin_report_matches_the_audit(ctx, kind):
    name = f"{kind}_m5"
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, _, rows, _ = case_data(name)
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
    got = ctx.bin_report(labels, B, m, rows)
    # confusion, unplaced, dcnt, dmin and n_skipped exactly; dsum by test_gpu_bin_report's criterion (its helper sums with
    # math.fsum, not in the kernel's order), which is relative and so holds at any scale
    check_report(name, got, expected(labels, B, rows, bins, dist))
    assert got[0].sum() + got[1].sum() + got[5] == len(rows) and 0 < got[5] < len(rows)
