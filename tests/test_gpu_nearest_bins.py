"""chb_audit_rows_nearest / chb_recruit_rows_nearest / clustering.nearest_bins: the k nearest bins of every row, ranked on
the device.

What the outputs are compared with:
  the dense call on the same context and arguments (chb_audit_rows, chb_audit_rows_grouped, chb_recruit_rows), ranked by
  test_nearest_bins_cpu.rank_dense -- the header's definition in numpy -- BITWISE (uint64 views), with the two identities
  the header states: slot 0 is bin_out / min_dist_out, slot 1 minus slot 0 is margin_out;
  and, independent of the dense call, row_reference.reference_rows: its finite distances sorted per row, elementwise
  within the row's largest row_reference.bound entry.  Sorting is 1-Lipschitz in the max norm -- if every entry of a row
  moves by at most e, so does every order statistic -- hence no entry is left out and there is no cap; the count of real
  slots is exact because the +inf pattern (empty bins) is.

Lane of the ranking kernel = bin % 16, 64 bins per round."""
import functools

import numpy as np
import pytest

import row_reference as RR
from test_gpu_many_bins import ROW_CASES, _bits_equal, _free_rows, _with_twins, row_data
from test_nearest_bins_cpu import rank_dense

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5
INF = np.inf


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check_shape_and_padding(nb, nd, k):
    """[Q, k] each; the real slots come first, padding is -1 / +inf, no NaN, (distance, bin) strictly ascending"""
    assert nb.shape == nd.shape and nb.shape[1] == k and nb.dtype == np.int64 and nd.dtype == np.float64
    pad = nb < 0
    assert np.all(nb[pad] == -1) and np.all(nd[pad] == INF) and np.all(np.isfinite(nd[~pad])) and not np.isnan(nd).any()
    cnt = (~pad).sum(axis=1)
    assert np.array_equal(pad, np.arange(k)[None, :] >= cnt[:, None])
    both = ~pad[:, 1:]
    d0, d1, b0, b1 = nd[:, :-1], nd[:, 1:], nb[:, :-1], nb[:, 1:]
    assert np.all((d0[both] < d1[both]) | ((d0[both] == d1[both]) & (b0[both] < b1[both])))
    return cnt


def check_against_dense(what, got, dense, k):
    """got = (near_bin, near_dist); dense = (bins, dist, min_dist, margin) of the dense call"""
    nb, nd = got
    bins, dist, mind, margin = dense
    cnt = check_shape_and_padding(nb, nd, k)
    wb, wd = rank_dense(dist, k)
    assert np.array_equal(nb, wb), what
    assert _bits_equal(nd, wd), what
    assert np.array_equal(cnt, np.minimum(np.isfinite(dist).sum(axis=1), k)), what
    assert np.array_equal(nb[:, 0], bins) and _bits_equal(np.ascontiguousarray(nd[:, 0]), mind), what
    if k >= 2:
        real = nb[:, 1] >= 0
        assert _bits_equal(nd[real, 1] - nd[real, 0], margin[real]), what
        if np.isfinite(dist).sum(axis=1).min() < 2:
            assert (~real).any()
        # (where slot 1 is padding the row has no finite runner-up)
        assert np.all(margin[~real] == INF), what


_dense = {}


def dense_calls(ctx, name, m, metric="convex"):
    """(audit_rows, recruit_rows) of a ROW_CASES case, once per (case, m, metric); leaves the case's samples resident"""
    X, labels, rows, Y = row_data(name)
    B = ROW_CASES[name]["B"]
    ctx.set_samples(X)
    key = (name, m, metric)
    if key not in _dense:
        with ctx.using_metric(metric):
            _dense[key] = (ctx.audit_rows(labels, B, m, rows), ctx.recruit_rows(labels, B, m, Y))
        for t in _dense[key]:
            for a in t:
                a.setflags(write=False)
    return _dense[key]


# ---- 1. bitwise against the dense call

# b9: nine lanes of a row hold a bin; b65: one bin past four loads of 16 (the second round holds one bin); b200: 3.1 rounds;
# b1100: +inf entries (empty bins); b8192: the limit, 36 % of the entries +inf
@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("name", list(ROW_CASES))
def test_bitwise_against_the_dense_call(ctx, name, k):
    c = ROW_CASES[name]
    B, m = c["B"], c["m"]
    X, labels, rows, Y = row_data(name)
    audit, recruit = dense_calls(ctx, name, m)
    check_against_dense(f"{name}/audit/k{k}", ctx.audit_rows_nearest(labels, B, m, k, rows), audit, k)
    check_against_dense(f"{name}/recruit/k{k}", ctx.recruit_rows_nearest(labels, B, m, k, Y), recruit, k)
    if name in ("b1100", "b8192"):
        assert np.isinf(audit[1]).any() and np.isinf(recruit[1]).any()
    if name == "b9" and k == 16:   # k > B pads
        assert np.all(ctx.audit_rows_nearest(labels, B, m, k, rows)[0][:, 9:] == -1)


@pytest.mark.parametrize("m,metric", [(1, "convex"), (16, "convex"), (5, "affine")])
def test_bitwise_other_neighbour_counts_and_the_affine_metric(ctx, m, metric):
    name, k = "b65", 5
    B = ROW_CASES[name]["B"]
    X, labels, rows, Y = row_data(name)
    audit, recruit = dense_calls(ctx, name, m, metric)
    with ctx.using_metric(metric):
        got_a = ctx.audit_rows_nearest(labels, B, m, k, rows)
        got_r = ctx.recruit_rows_nearest(labels, B, m, k, Y)
    check_against_dense(f"{name}/audit/m{m}/{metric}", got_a, audit, k)
    check_against_dense(f"{name}/recruit/m{m}/{metric}", got_r, recruit, k)
    if metric == "affine":   # (the metric reached the kernel: the affine hull is nearer than the convex one somewhere)
        assert not _bits_equal(got_a[1], ctx.audit_rows_nearest(labels, B, m, k, rows)[1])


# ---- 2. grouped

def test_grouped(ctx):
    name, k = "b65", 5
    c = ROW_CASES[name]
    B, m = c["B"], c["m"]
    X, labels, rows, _ = row_data(name)
    groups = np.arange(len(X), dtype=np.int64) // 4   # four pieces per parent
    ctx.set_samples(X)
    dense = ctx.audit_rows_grouped(labels, groups, B, m, rows)
    got = ctx.audit_rows_nearest(labels, B, m, k, rows, groups=groups)
    check_against_dense("grouped", got, dense, k)
    plain = ctx.audit_rows_nearest(labels, B, m, k, rows)
    check_against_dense("groups=None", plain, dense_calls(ctx, name, m)[0], k)


# ---- 3. exact ties

def test_zero_ties_go_to_the_lower_bin(ctx):
    """test_gpu_many_bins.test_exact_zero_ties' construction: five bins hold a twin of the scored row.  Lanes: 3, 11, 3
    (bin 19, the second load), 5, 12."""
    B, m, twin_bins = 200, 5, (3, 11, 19, 5, 12)
    X, labels, s, Y = _with_twins(twin_bins)
    ctx.set_samples(X)
    rows = np.array([s, s + 1, s], dtype=np.int64)
    for k in (5, 16, 2):
        for what, got, dense in (("audit", ctx.audit_rows_nearest(labels, B, m, k, rows), ctx.audit_rows(labels, B, m, rows)),
                                 ("recruit", ctx.recruit_rows_nearest(labels, B, m, k, Y), ctx.recruit_rows(labels, B, m, Y))):
            check_against_dense(f"zero ties/{what}/k{k}", got, dense, k)
            nb, nd = got
            t = min(k, 5)
            assert nb[0, :t].tolist() == sorted(twin_bins)[:t], (what, nb[0])
            assert np.all(nd[0, :t] == 0.0) and not np.signbit(nd[0, :t]).any()
            if k > 5:
                assert nd[0, 5] > 0.0
            if what == "audit":
                assert np.array_equal(nb[2], nb[0]) and _bits_equal(nd[2], nd[0])


def identical_bins(a, others):
    """test_gpu_many_bins.test_nonzero_tie_between_identical_bins' construction for any number of copies: every bin of
    `others` gets bin a's member set through duplicated rows, in the same index order.  -> (X, labels, near, Y)"""
    X0, labels0, _, Y0 = row_data("b200")
    X, labels = X0.copy(), labels0.copy()
    labels[np.isin(labels, others)] = -1
    near = np.flatnonzero(labels == a)[-6:]   # six of bin a's own members, taken out of it: the rows to score
    labels[near] = -1
    mem_a = np.flatnonzero(labels == a)
    assert len(mem_a) >= 5
    taken = set(near.tolist())
    for b in others:
        copies = _free_rows(labels, taken, len(mem_a))
        X[copies] = X[mem_a]
        labels[copies] = b
        taken |= set(copies.tolist())
    return X, labels, near.astype(np.int64), np.vstack([X[near], Y0[:10]])


# (24, 40): lane 8 twice, two loads of one round; (52, 30): lanes 4 and 14, the lower bin in the higher lane;
# (24, 45, 99): lanes 8, 13 and 3, the last in the second round
@pytest.mark.parametrize("a,others", [(24, (40,)), (52, (30,)), (24, (45, 99))], ids=["same_lane", "other_lanes", "three_way"])
def test_nonzero_ties_between_identical_bins(ctx, a, others):
    B, m, k = 200, 5, 5
    tied_bins = sorted((a,) + others)
    assert len({b % 16 for b in tied_bins}) == (1 if others == (40,) else len(tied_bins))
    X, labels, near, Y = identical_bins(a, others)
    ctx.set_samples(X)
    for what, got, dense in (("audit", ctx.audit_rows_nearest(labels, B, m, k, near), ctx.audit_rows(labels, B, m, near)),
                             ("recruit", ctx.recruit_rows_nearest(labels, B, m, k, Y), ctx.recruit_rows(labels, B, m, Y))):
        check_against_dense(f"ties/{what}", got, dense, k)
        nb, nd = got
        dist = dense[1]
        for b in others:
            assert _bits_equal(np.ascontiguousarray(dist[:, a]), np.ascontiguousarray(dist[:, b])), what
        tied = dist[:, a] == dist.min(axis=1)
        assert tied.sum() >= 3, (what, tied.sum())
        t = len(tied_bins)
        assert np.all(nb[tied, :t] == np.array(tied_bins)) and np.all(nd[tied, 0] > 0.0), what
        for j in range(1, t):   # adjacent slots, equal bits
            assert _bits_equal(np.ascontiguousarray(nd[tied, j]), np.ascontiguousarray(nd[tied, 0])), what
        # wherever the tied bins appear at all they are adjacent and ascending
        for q in range(len(nb)):
            at = np.flatnonzero(np.isin(nb[q], tied_bins))
            assert np.array_equal(at, np.arange(at[0], at[0] + len(at))) if len(at) else True
            assert nb[q, at].tolist() == tied_bins[:len(at)]


# ---- 4. few finite entries

@pytest.mark.parametrize("keep", [(15,), (6, 22), (199,)], ids=["one", "two_same_lane", "last_bin"])
def test_rows_with_one_or_two_finite_bins(ctx, keep):
    B, m, k = 200, 5, 3
    X, labels0, rows, Y = row_data("b200")
    labels = np.where(np.isin(labels0, keep), labels0, -1)
    ctx.set_samples(X)
    for got, dense in ((ctx.audit_rows_nearest(labels, B, m, k, rows), ctx.audit_rows(labels, B, m, rows)),
                       (ctx.recruit_rows_nearest(labels, B, m, k, Y), ctx.recruit_rows(labels, B, m, Y))):
        check_against_dense(f"keep{keep}", got, dense, k)
        nb, nd = got
        n = len(keep)
        assert np.all(np.sort(nb[:, :n], axis=1) == np.array(keep)) and np.all(nb[:, n:] == -1) and np.all(nd[:, n:] == INF)
        assert np.all(np.isfinite(nd[:, :n]))
        if n == 2:
            assert len(set(nb[:, 0].tolist())) == 2   # (each of the two is nearest somewhere)


def test_no_finite_entry_one_bin_and_k_beyond_b(ctx):
    X, labels0, rows, Y = row_data("b9")
    m = 5
    ctx.set_samples(X)
    # no labelled sample at all: every slot is padding
    none = np.full(len(X), -1, dtype=np.int64)
    for nb, nd in (ctx.audit_rows_nearest(none, 9, m, 3, rows), ctx.recruit_rows_nearest(none, 9, m, 3, Y)):
        assert nb.shape == (len(rows), 3) and np.all(nb == -1) and np.all(nd == INF)
    # B = 1 with k = 1
    one = np.where(labels0 >= 0, 0, -1)
    check_against_dense("B1/audit", ctx.audit_rows_nearest(one, 1, m, 1, rows), ctx.audit_rows(one, 1, m, rows), 1)
    nb, nd = ctx.recruit_rows_nearest(one, 1, m, 1, Y)
    check_against_dense("B1/recruit", (nb, nd), ctx.recruit_rows(one, 1, m, Y), 1)
    assert np.all(nb == 0) and np.all(np.isfinite(nd))
    # B = 3 with k = 16: three real slots, thirteen of padding
    three = np.where(labels0 >= 0, labels0 % 3, -1)
    nb, nd = ctx.audit_rows_nearest(three, 3, m, 16, rows)
    check_against_dense("B3/audit", (nb, nd), ctx.audit_rows(three, 3, m, rows), 16)
    assert np.all(np.sort(nb[:, :3], axis=1) == np.arange(3)) and np.all(nb[:, 3:] == -1) and np.all(nd[:, 3:] == INF)
    check_against_dense("B3/recruit", ctx.recruit_rows_nearest(three, 3, m, 16, Y), ctx.recruit_rows(three, 3, m, Y), 16)


# ---- 5. chunk edge

@functools.lru_cache(maxsize=None)
def chunk_data():
    from chbin_amd import synth
    N, D, B, m = 700, 8, 5, 3
    X, _, true = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    labels = true.copy()
    labels[np.random.default_rng(3).random(N) < 0.3] = -1
    return np.ascontiguousarray(X), labels, B, m


def test_chunk_edge_audit(ctx):
    """chunk + 70 positions cycling through the samples: both halves of the double buffer, and a last chunk of 70 rows --
    four full groups of 16 and one of 6, whose other lanes' rows store nothing."""
    chunk = ctx.counter("recruit_chunk")
    assert chunk == 16384 and 70 % 16 != 0
    X, labels, B, m = chunk_data()
    N, k = len(X), 3
    Q = chunk + 70
    rows = (np.arange(Q) % N).astype(np.int64)
    ctx.set_samples(X)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.audit_rows_nearest(labels, B, m, k, rows)
    pa, pn, pr = ctx.profile_get("audit"), ctx.profile_get("nearest_bins"), ctx.profile_get("recruit")
    ctx.profile_enable(False)
    assert pa["launches"] == 2 and pn["launches"] == 2 and pa["work"] == Q * B and pn["work"] == Q * B and pr["launches"] == 0
    check_against_dense("chunk/audit", got, ctx.audit_rows(labels, B, m, rows), k)
    assert np.array_equal(got[0], got[0][:N][rows]) and _bits_equal(got[1], got[1][:N][rows])
    # rows=None is the same call as rows = 0 .. N-1
    for a, b in zip(ctx.audit_rows_nearest(labels, B, m, k), got):
        assert _bits_equal(a, np.ascontiguousarray(b[:N]))


def test_chunk_edge_recruit(ctx):
    X, labels, B, m = chunk_data()
    N, k = len(X), 3
    Q = ctx.counter("recruit_chunk") + 70
    rng = np.random.default_rng(4)
    Y = X[np.arange(Q) % N] + 1e-3 * rng.standard_normal((Q, X.shape[1]))
    ctx.set_samples(X)
    got = ctx.recruit_rows_nearest(labels, B, m, k, Y)
    check_against_dense("chunk/recruit", got, ctx.recruit_rows(labels, B, m, Y), k)


# ---- 6. independent of the dense call

def test_against_the_row_reference(ctx):
    from chbin_amd import synth
    N, D, B, m, Q, k = 600, 16, 7, 5, 40, 4
    Z, _, true = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    rng = np.random.default_rng(7)
    labels = true[:N].copy()
    labels[rng.random(N) < 0.3] = -1
    labels[labels == 6] = -1   # an empty bin: six finite entries per row
    rows = np.sort(rng.choice(N, Q, replace=False)).astype(np.int64)
    ctx.set_samples(X)
    for what, (nb, nd), ref in (("audit", ctx.audit_rows_nearest(labels, B, m, k, rows), RR.reference_rows(X, labels, B, m, rows=rows)),
                                ("recruit", ctx.recruit_rows_nearest(labels, B, m, k, Y), RR.reference_rows(X, labels, B, m, Y=Y))):
        cnt = check_shape_and_padding(nb, nd, k)
        fin = np.isfinite(ref.dist)
        assert np.array_equal(cnt, np.minimum(fin.sum(axis=1), k)), what   # exact
        assert np.all(fin.sum(axis=1) == 6)
        want = np.sort(np.where(fin, ref.dist, INF), axis=1)[:, :k]
        tol = RR.bound(ref).max(axis=1)
        err = np.abs(nd - want)
        print(f"{what}: largest |near_dist - sorted reference| = {err.max():.3e}, smallest bound {tol.min():.3e}")
        assert np.all(err <= tol[:, None]), (what, (err / tol[:, None]).max())
        assert not np.isin(nb, [6]).any()


# ---- 7. optional outputs and guards, through the raw ABI

def ptr(a):
    return None if a is None else a.ctypes.data


def raw_audit(ctx, labels, groups, B, m, k, rows, Q, nb, nd):
    return ctx._lib.chb_audit_rows_nearest(ctx._h, ptr(labels), ptr(groups), B, m, k, ptr(rows), Q, ptr(nb), ptr(nd))


def raw_recruit(ctx, labels, B, m, k, Y, Q, D, nb, nd):
    return ctx._lib.chb_recruit_rows_nearest(ctx._h, ptr(labels), B, m, k, ptr(Y), Q, D, ptr(nb), ptr(nd))


def outputs(Q, k, extra=7):
    return np.full(Q * k + extra, -55, dtype=np.int64), np.full(Q * k + extra, -5.0)


def untouched(out, n):
    return np.all(out[0][n:] == -55) and np.all(out[1][n:] == -5.0)


def test_optional_outputs_and_guards(ctx):
    name, k = "b65", 5
    c = ROW_CASES[name]
    B, m, Q = c["B"], c["m"], c["Q"]
    X, labels, rows, Y = row_data(name)
    ctx.set_samples(X)
    full_a = ctx.audit_rows_nearest(labels, B, m, k, rows)
    full_r = ctx.recruit_rows_nearest(labels, B, m, k, Y)
    groups = np.arange(len(X), dtype=np.int64) // 4
    full_g = ctx.audit_rows_nearest(labels, B, m, k, rows, groups=groups)
    D = X.shape[1]
    for mask in (1, 2, 3):
        for full, call in ((full_a, lambda nb, nd: raw_audit(ctx, labels, None, B, m, k, rows, Q, nb, nd)),
                           (full_g, lambda nb, nd: raw_audit(ctx, labels, groups, B, m, k, rows, Q, nb, nd)),
                           (full_r, lambda nb, nd: raw_recruit(ctx, labels, B, m, k, Y, Q, D, nb, nd))):
            out = outputs(Q, k)
            assert call(out[0] if mask & 1 else None, out[1] if mask & 2 else None) == 0, mask
            assert untouched(out, Q * k)   # the guard elements behind Q * k
            if mask & 1:
                assert np.array_equal(out[0][:Q * k], full[0].reshape(-1))
            else:
                assert np.all(out[0] == -55)
            if mask & 2:
                assert _bits_equal(out[1][:Q * k], full[1].reshape(-1))
            else:
                assert np.all(out[1] == -5.0)


# ---- 8. refusals

def test_abi_refusals_in_order():
    """Every rule of the header with its code; where two rules are broken at once the earlier check answers (the order of
    score_check_args: ranges, null arguments, outputs, samples, D, m > 16, k > 16, B > 8192, an open fit, Q = 0, row_idx)."""
    import test_gpu_recruit as R
    from chbin_amd import _lib
    c = R.CASES["base"]
    X, labels, Y = R.case_data("base")
    N, D, B, m, Q = c["N"], c["D"], c["B"], c["m"], c["Q"]
    k = 3
    rows = np.arange(0, N, 7, dtype=np.int64)
    P = len(rows)
    groups = np.arange(N, dtype=np.int64) // 3
    out = outputs(max(P, Q), 17, extra=0)
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib
        A = lambda *a: raw_audit(ctx, *a)
        Rc = lambda *a: raw_recruit(ctx, *a)

        def refused(rc, code, text=None):
            assert rc == code, (rc, code, lib.chb_last_error())
            assert untouched(out, 0)   # nothing was written
            if text is not None:
                assert text in lib.chb_last_error(), lib.chb_last_error()

        # without samples: CHB_ESTATE, but the checks in front of it answer first
        refused(A(labels, None, B, m, k, rows, P, *out), ESTATE)
        refused(Rc(labels, B, m, k, Y, Q, D, *out), ESTATE)
        refused(A(labels, None, B, m, 0, rows, P, *out), EINVAL, b"k < 1")
        refused(A(labels, None, B, m, k, rows, P, None, None), EINVAL, b"both null")
        refused(A(None, None, B, m, k, rows, P, *out), EINVAL)
        refused(A(labels, None, B, 17, k, rows, P, *out), ESTATE)     # (the limits come behind the state)
        refused(Rc(labels, B, m, 17, Y, Q, D, *out), ESTATE)
        ctx.set_samples(X)
        ref_a = ctx.audit_rows_nearest(labels, B, m, k, rows)
        ref_g = ctx.audit_rows_nearest(labels, B, m, k, rows, groups=groups)
        ref_r = ctx.recruit_rows_nearest(labels, B, m, k, Y)

        def usable():   # the context still answers, and with the same bits
            for got, ref in ((ctx.audit_rows_nearest(labels, B, m, k, rows), ref_a),
                             (ctx.audit_rows_nearest(labels, B, m, k, rows, groups=groups), ref_g),
                             (ctx.recruit_rows_nearest(labels, B, m, k, Y), ref_r)):
                assert np.array_equal(got[0], ref[0]) and _bits_equal(got[1], ref[1])

        # null context, ranges (k among them), null arguments
        refused(lib.chb_audit_rows_nearest(None, ptr(labels), None, B, m, k, ptr(rows), P, ptr(out[0]), ptr(out[1])), EINVAL)
        refused(lib.chb_recruit_rows_nearest(None, ptr(labels), B, m, k, ptr(Y), Q, D, ptr(out[0]), ptr(out[1])), EINVAL)
        for g in (None, groups):
            refused(A(labels, g, B, m, k, rows, -1, *out), EINVAL)
            refused(A(labels, g, 0, m, k, rows, P, *out), EINVAL)
            refused(A(labels, g, B, 0, k, rows, P, *out), EINVAL)
            refused(A(labels, g, B, m, 0, rows, P, *out), EINVAL, b"k < 1")
            refused(A(labels, g, B, m, -3, rows, P, *out), EINVAL, b"k < 1")
            refused(A(None, g, B, m, k, rows, P, *out), EINVAL, b"null argument")
            refused(A(labels, g, B, m, k, rows, P, None, None), EINVAL, b"both null")
        refused(Rc(labels, B, m, k, Y, -1, D, *out), EINVAL)
        refused(Rc(labels, 0, m, k, Y, Q, D, *out), EINVAL)
        refused(Rc(labels, B, 0, k, Y, Q, D, *out), EINVAL)
        refused(Rc(labels, B, m, 0, Y, Q, D, *out), EINVAL, b"k < 1")
        refused(Rc(None, B, m, k, Y, Q, D, *out), EINVAL, b"null argument")
        refused(Rc(labels, B, m, k, None, Q, D, *out), EINVAL, b"null argument")
        refused(Rc(labels, B, m, k, Y, Q, D, None, None), EINVAL, b"both null")
        refused(A(labels, None, B, m, 0, rows, P, None, None), EINVAL, b"k < 1")          # the range before the outputs
        refused(A(labels, None, B, 17, 0, rows, P, *out), EINVAL, b"k < 1")               # ... and before the limits
        refused(A(labels, None, B, m, 17, rows, P, None, None), EINVAL, b"both null")     # the outputs before the limits
        usable()
        # D
        refused(Rc(labels, B, m, k, Y, Q, D - 1, *out), EINVAL, b"columns")
        refused(Rc(labels, B, m, k, Y, Q, D + 1, *out), EINVAL, b"columns")
        refused(Rc(labels, B, 17, k, Y, Q, D + 1, *out), EINVAL, b"columns")              # D before the limits
        # limits: m > 16, right behind it k > 16, then B > 8192
        for g in (None, groups):
            refused(A(labels, g, B, 17, k, rows, P, *out), EUNSUPPORTED, b"neighbours")
            refused(A(labels, g, B, m, 17, rows, P, *out), EUNSUPPORTED, b"nearest bins")
            refused(A(labels, g, 8193, m, k, rows, P, *out), EUNSUPPORTED, b"8192")
            refused(A(labels, g, 8193, 17, 17, rows, P, *out), EUNSUPPORTED, b"neighbours")
            refused(A(labels, g, 8193, m, 17, rows, P, *out), EUNSUPPORTED, b"nearest bins")
        refused(Rc(labels, B, 17, k, Y, Q, D, *out), EUNSUPPORTED, b"neighbours")
        refused(Rc(labels, B, m, 17, Y, Q, D, *out), EUNSUPPORTED, b"nearest bins")
        refused(Rc(labels, 8193, m, k, Y, Q, D, *out), EUNSUPPORTED, b"8192")
        refused(Rc(labels, 8193, m, 17, Y, Q, D, *out), EUNSUPPORTED, b"nearest bins")
        bad = rows.copy()
        bad[P // 2] = N
        refused(A(labels, None, 8193, m, k, bad, P, *out), EUNSUPPORTED, b"8192")         # the limits before row_idx
        refused(A(labels, None, B, m, 17, None, N - 1, *out), EUNSUPPORTED, b"nearest bins")
        assert A(labels, None, B, 16, 16, rows, 3, *outputs(3, 16)) == 0                 # the limits themselves are served
        usable()
        # row_idx: NULL means all rows and Q must be N; entries in [0, N)
        assert A(labels, None, B, m, k, None, N, *outputs(N, k)) == 0
        refused(A(labels, None, B, m, k, None, N - 1, *out), EINVAL, b"row_idx")
        refused(A(labels, groups, B, m, k, None, N + 1, *out), EINVAL, b"row_idx")
        for v in (-1, N):
            bad = rows.copy()
            bad[P - 1] = v
            refused(A(labels, None, B, m, k, bad, P, *out), EINVAL, b"row_idx")
            refused(A(labels, groups, B, m, k, bad, P, *out), EINVAL, b"row_idx")
        usable()
        # Q = 0: CHB_OK, nothing is read or written (with NULL row_idx too)
        refused(A(None, None, B, m, k, None, 0, *out), 0)
        refused(A(labels, groups, B, m, k, rows, 0, *out), 0)
        refused(Rc(None, B, m, k, None, 0, D, *out), 0)
        empty = ctx.audit_rows_nearest(labels, B, m, k, np.zeros(0, dtype=np.int64))
        assert empty[0].shape == (0, k) and empty[1].shape == (0, k)
        usable()
    finally:
        ctx.close()


# ---- 9. no trace

def test_no_trace_left_in_a_fit():
    """fit_cluster, the nearest-bins calls, the same fit again on one context: labels, sweeps and change counts identical,
    every counter and the fit statistics as without the calls in between."""
    from chbin_amd import _lib, synth
    from test_gpu_pairs import COUNTERS
    names = COUNTERS + ("pair_tiles",)
    N, D, B, m, its, k = 2500, 136, 8, 5, 3, 3
    Z, initial, _ = synth.make_synthetic(N + 200, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    initial = initial[:N].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    groups = np.arange(N, dtype=np.int64) // 2

    def two_fits(calls_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for j in range(2):
                lab, sweeps, changed = ctx.fit_cluster(B, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in names], ctx.fit_stats()))
                if j == 0 and calls_between:
                    nb, nd = ctx.audit_rows_nearest(lab, B, m, k)
                    assert np.all(nb >= 0) and np.isfinite(nd).all()
                    assert np.all(ctx.audit_rows_nearest(lab, B, m, k, groups=groups)[0] >= 0)
                    assert np.all(ctx.recruit_rows_nearest(lab, B, m, k, Y)[0] >= 0)
                    assert [ctx.counter(n) for n in names] == res[0][3]
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


def test_refused_while_a_stepwise_fit_is_open():
    """CHB_ESTATE at every stage of an open stepwise fit, and the fit completes with the labels it gives undisturbed."""
    import test_gpu_recruit as R
    from chbin_amd import _lib, synth
    c = R.CASES["base"]
    X, labels, Y = R.case_data("base")
    N, D, B, m, Q = c["N"], c["D"], c["B"], c["m"], c["Q"]
    k = 3
    rows = np.arange(0, N, 7, dtype=np.int64)
    P = len(rows)
    groups = np.arange(N, dtype=np.int64) // 3
    out = outputs(max(P, Q), k, extra=0)
    _, initial, _ = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    initial = initial[:N].copy()
    sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
    ctx, other = _lib.Context(0), _lib.Context(0)
    try:
        ctx.set_samples(X)
        other.set_samples(X)
        ref = ctx.audit_rows_nearest(labels, B, m, k, rows)

        def refused(rc):
            assert rc == ESTATE, (rc, ctx._lib.chb_last_error())
            assert untouched(out, 0) and b"stepwise" in ctx._lib.chb_last_error()

        res = {}
        for who, cx in (("disturbed", ctx), ("plain", other)):
            cx.fit_begin(B, initial, m)
            if who == "disturbed":
                refused(raw_audit(ctx, labels, None, B, m, k, rows, P, *out))
            cx.batch_begin(sl, 0, len(sl))
            guess = np.full(len(sl), -1, dtype=np.int64)
            cx.batch_guess(guess)
            lab1, md1 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(guess, 0, lab1, md1)
            if who == "disturbed":
                refused(raw_audit(ctx, labels, groups, B, m, k, rows, P, *out))
                refused(raw_recruit(ctx, labels, B, m, k, Y, Q, D, *out))
            lab2, md2 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(lab1, 0, lab2, md2)
            cx.batch_commit(lab2)
            res[who] = (lab1, lab2, cx.fit_labels())
        for a, b in zip(res["disturbed"], res["plain"]):
            assert np.array_equal(a, b)
        assert np.all(res["plain"][1] >= 0)
        ctx.set_samples(X)   # ends the stepwise fit
        got = ctx.audit_rows_nearest(labels, B, m, k, rows)
        assert np.array_equal(got[0], ref[0]) and _bits_equal(got[1], ref[1])
    finally:
        ctx.close()
        other.close()


# ---- 10. the Python mirror

@pytest.mark.parametrize("name", ["small_and_empty_bins", "affine"])
def test_mirror_functions(ctx, name):
    from chbin_amd import _lib, clustering
    from test_gpu_audit import CASES, case_data
    c = CASES[name]
    B, m, metric = c["B"], c["m"], c.get("metric", "convex")
    X, labels, _ = case_data(name)
    k = 3
    rows = np.arange(3, len(X), 5, dtype=np.int64)
    ctx.set_samples(X)
    with ctx.using_metric(metric):
        dense = ctx.audit_rows(labels, B, m, rows)
        want = ctx.audit_rows_nearest(labels, B, m, k, rows)
    got = clustering.nearest_bins(X, labels, B, k=k, num_neighbors=m, metric=metric, rows=rows)
    assert isinstance(got, clustering.NearestBins)
    assert np.array_equal(got.bins, want[0]) and _bits_equal(got.dist, want[1])
    assert _lib.default_context().get_metric() == "convex"
    check_against_dense(f"mirror/{name}", (got.bins, got.dist), dense, k)
    assert np.array_equal(got.count, (got.bins >= 0).sum(axis=1))
    assert _bits_equal(got.margin, dense[3])   # audit's margin bit for bit, +inf included
    if name == "small_and_empty_bins":   # four bins with members enough, one of one, one of two, one of none: never 7 finite
        assert got.count.max() == k and np.all(np.isfinite(dense[1]).sum(axis=1) < B)
    pos, bins = got.pairs(ranks=(0, 1))
    assert len(pos) == 2 * len(rows) and np.array_equal(pos, np.repeat(np.arange(len(rows)), 2))
    with ctx.using_metric(metric):
        pd = ctx.audit_pairs(labels, B, m, rows[pos], bins)
    assert _bits_equal(pd, got.dist[:, :2].reshape(-1))   # the pairs are what audit_pairs takes
    amb = got.ambiguous(0.05, relative=True)
    assert amb.dtype == bool and np.array_equal(amb, got.margin <= 0.05 * got.dist[:, 0])
    # all rows, with groups
    groups = np.arange(len(X), dtype=np.int64) // 4
    gg = clustering.nearest_bins(X, labels, B, k=k, num_neighbors=m, metric=metric, groups=groups)
    ctx.set_samples(X)
    with ctx.using_metric(metric):
        wg = ctx.audit_rows_nearest(labels, B, m, k, groups=groups)
    assert gg.bins.shape == (len(X), k) and np.array_equal(gg.bins, wg[0]) and _bits_equal(gg.dist, wg[1])
    # the recruit form
    rng = np.random.default_rng(41)
    Y = np.ascontiguousarray(X[rng.choice(len(X), 50, replace=False)] + 1e-3 * rng.standard_normal((50, X.shape[1])))
    gr = clustering.recruit_nearest_bins(X, labels, Y, B, k=k, num_neighbors=m, metric=metric)
    ctx.set_samples(X)
    with ctx.using_metric(metric):
        check_against_dense(f"mirror/recruit/{name}", (gr.bins, gr.dist), ctx.recruit_rows(labels, B, m, Y), k)
    pos, bins = gr.pairs(ranks=(0,))
    with ctx.using_metric(metric):
        assert _bits_equal(ctx.recruit_pairs(labels, B, m, Y, pos, bins), np.ascontiguousarray(gr.dist[:, 0]))
