"""chb_audit_pairs_witness / chb_recruit_pairs_witness / clustering.witness: the pair calls' distances together with the hull
each was measured to -- the members' sample indices, their selection distances, their weights.

What the outputs are compared with:
  dist           the plain pair call on the same context, BITWISE (uint64 views);
  nbr_idx/dist   chb_topm_per_bin's [row, bin] lists and chb_pairwise_distance's entries, bitwise (both share the
                 selection's arithmetic and (distance, index) order by their headers); for the grouped call the same on
                 the labels with the row's group set to -1 (the grouped calls' definition, groups_reference.py); for new
                 rows the index sets of row_reference.reference_rows (the oracle's cdist row + find_nearest_from_cluster);
  alpha          the project's rule for a weight vector (test_gpu_parity.py:149-151, 297-298): feasible, and
                 | ||alpha @ X[nbr] - y|| - dist | <= QP_TOL + 1e-7 scale (dist < 1e-6 scale), scale = the pair's largest
                 selection distance.  Reconstruction does not need the weights to be unique, so the cases with twins
                 (m16_dups) and with 15 / 16 vertices are held to it like the others."""
import functools

import numpy as np
import pytest

import groups_reference as G
import row_reference as RR
from test_gpu_audit import CASES, QP_TOL, case_data

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -4, -5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bitwise equality of two tuples of arrays (float64 by their bits, int64 as they are)"""
    return all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_memo = {}


def case_witness(ctx, name):
    """One witness call per case, shared by the tests: every (row, bin) pair of the case's rows, shuffled, a fifth of them
    twice.  -> dict(rows, bins, plain, w = (dist, idx, nd, alpha), topm = (idx, dist, cnt) over the unique rows, upos)"""
    if name in _memo:
        return _memo[name]
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, crow = case_data(name)
    uniq = np.arange(len(X)) if crow is None else np.unique(crow)
    rng = np.random.default_rng(31)
    grid = np.stack(np.meshgrid(uniq, np.arange(B), indexing="ij"), axis=-1).reshape(-1, 2)
    grid = np.concatenate([grid, grid[rng.choice(len(grid), len(grid) // 5, replace=False)]])
    grid = grid[rng.permutation(len(grid))]
    rows, bins = np.ascontiguousarray(grid[:, 0]), np.ascontiguousarray(grid[:, 1])
    ctx.set_samples(X)
    with ctx.using_metric(c.get("metric", "convex")):
        plain = ctx.audit_pairs(labels, B, m, rows, bins)
        w = ctx.audit_pairs_witness(labels, B, m, rows, bins)
    topm = ctx.topm_per_bin(labels, B, m, uniq)
    pd = ctx.pairwise_distance()
    for a in (plain, pd) + tuple(w) + tuple(topm):
        a.setflags(write=False)
    _memo[name] = dict(rows=rows, bins=bins, plain=plain, w=w, topm=topm, upos=np.searchsorted(uniq, rows), pd=pd)
    return _memo[name]


@functools.lru_cache(maxsize=None)
def recruit_data(name):
    """(X, labels, Y, row_of, bins) of a recruit case on the audit's samples: 48 rows perturbed off samples, 8 exact copies
    of samples (labelled and not), every bin for each, shuffled with repeats."""
    c = CASES[name]
    X, labels, _ = case_data(name)
    rng = np.random.default_rng(32)
    src = rng.choice(len(X), 56, replace=False)
    Y = X[src].copy()
    Y[:48] += 2e-3 * rng.standard_normal((48, X.shape[1])) / X.shape[1]
    Y = np.ascontiguousarray(Y)
    grid = np.stack(np.meshgrid(np.arange(56), np.arange(c["B"]), indexing="ij"), axis=-1).reshape(-1, 2)
    grid = np.concatenate([grid, grid[:40]])[rng.permutation(len(grid) + 40)]
    return X, labels, Y, np.ascontiguousarray(grid[:, 0]), np.ascontiguousarray(grid[:, 1]), src


@functools.lru_cache(maxsize=None)
def recruit_reference(name):
    c = CASES[name]
    X, labels, Y, _, _, _ = recruit_data(name)
    return RR.reference_rows(X, labels, c["B"], c["m"], Y=Y, want_sets=True)


def check_padding(idx, nd, alpha):
    pad = idx < 0
    assert np.all(idx[pad] == -1) and np.all(nd[pad] == np.inf) and np.all(alpha[pad] == 0.0)
    cnt = (~pad).sum(axis=1)
    assert np.array_equal(pad, np.arange(idx.shape[1])[None, :] >= cnt[:, None])   # the real slots come first
    assert np.all(np.isfinite(nd[~pad])) and not np.isnan(alpha).any()
    return cnt


# ---- 1. dist is the plain call's

@pytest.mark.parametrize("name", list(CASES))
def test_dist_is_the_plain_calls_bitwise(ctx, name):
    w = case_witness(ctx, name)
    assert w["w"][0].shape == w["plain"].shape and len(np.unique(w["rows"] * 64 + w["bins"])) < len(w["rows"])
    assert np.array_equal(bits(w["w"][0]), bits(w["plain"]))
    assert np.isinf(w["plain"]).any() or name not in ("small_and_empty_bins",)


def test_dist_grouped_bitwise(ctx):
    X, labels, groups = G.group_data()
    rng = np.random.default_rng(33)
    order = rng.permutation(G.N * G.B)
    order = np.concatenate([order, order[:300]])
    rows, bins = order // G.B, order % G.B
    ctx.set_samples(X)
    plain = ctx.audit_pairs_grouped(labels, groups, G.B, 5, rows, bins)
    dist, idx, nd, alpha = ctx.audit_pairs_witness(labels, G.B, 5, rows, bins, groups=groups)
    assert np.array_equal(bits(dist), bits(plain)) and np.isinf(plain).any()
    check_padding(idx, nd, alpha)
    # ... and without groups the same call is the ungrouped one
    assert np.array_equal(bits(ctx.audit_pairs_witness(labels, G.B, 5, rows, bins)[0]),
                          bits(ctx.audit_pairs(labels, G.B, 5, rows, bins)))


@pytest.mark.parametrize("name", ["base", "wide_d300"])
def test_dist_recruit_bitwise(ctx, name):
    c = CASES[name]
    X, labels, Y, row_of, bins, _ = recruit_data(name)
    ctx.set_samples(X)
    plain = ctx.recruit_pairs(labels, c["B"], c["m"], Y, row_of, bins)
    dist = ctx.recruit_pairs_witness(labels, c["B"], c["m"], Y, row_of, bins)[0]
    assert np.array_equal(bits(dist), bits(plain))
    assert np.count_nonzero(plain == 0.0) >= 4   # the copies of labelled samples against their own bins


# ---- 2. the index lists are the selection's

@pytest.mark.parametrize("name", list(CASES))
def test_lists_are_topm_per_bin(ctx, name):
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data(name)
    w = case_witness(ctx, name)
    rows, bins, upos = w["rows"], w["bins"], w["upos"]
    dist, idx, nd, alpha = w["w"]
    t_idx, t_dist, t_cnt = w["topm"]
    assert idx.shape == nd.shape == alpha.shape == (len(rows), m)
    assert np.array_equal(idx, t_idx[upos, bins])
    assert np.array_equal(bits(nd), bits(t_dist[upos, bins]))
    cnt = check_padding(idx, nd, alpha)
    assert np.array_equal(cnt, t_cnt[upos, bins])
    assert np.array_equal(np.isinf(dist), cnt == 0)
    # chb_pairwise_distance's entries, bit for bit
    real = idx >= 0
    pd = w["pd"]
    assert np.array_equal(bits(nd[real]), bits(pd[np.broadcast_to(rows[:, None], idx.shape)[real], idx[real]]))
    # members of the pair's bin, never the row itself, (distance, index) ascending
    assert np.all(labels[idx[real]] == np.broadcast_to(bins[:, None], idx.shape)[real])
    assert not np.any(idx == rows[:, None])
    d0, d1, i0, i1 = nd[:, :-1], nd[:, 1:], idx[:, :-1], idx[:, 1:]
    both = real[:, 1:]
    assert np.all((d0[both] < d1[both]) | ((d0[both] == d1[both]) & (i0[both] < i1[both])))

    if name == "m16_dups":
        # ties are broken by index, and a twin stays (the index is withheld, not distance 0)
        assert np.count_nonzero((d0 == d1) & both) > 50
        twin = nd[:, 0] == 0.0
        assert np.count_nonzero(twin) > 50
        assert np.all(X[idx[twin, 0]] == X[rows[twin]]) and np.all(idx[twin, 0] != rows[twin])
        assert np.count_nonzero(twin & (labels[rows] == bins)) > 10
    if name == "small_and_empty_bins":
        one, two, none = B - 3, B - 2, B - 1
        lone = np.flatnonzero(labels == one)[0]
        assert np.all(cnt[bins == none] == 0) and np.all(dist[bins == none] == np.inf)
        assert np.all(cnt[(bins == one) & (rows != lone)] == 1) and np.all(cnt[(bins == one) & (rows == lone)] == 0)
        pair = np.flatnonzero(labels == two)
        assert np.all(cnt[(bins == two) & ~np.isin(rows, pair)] == 2) and np.all(cnt[(bins == two) & np.isin(rows, pair)] == 1)
        assert set(np.unique(cnt)) >= {0, 1, 2, m}


def test_lists_grouped_are_topm_on_the_labels_without_the_group(ctx):
    X, labels, groups = G.group_data()
    m = 5
    by = lambda g: np.flatnonzero(groups == g)
    rng = np.random.default_rng(34)
    chosen = np.concatenate([by(G.BIG)[:6], by(G.ALL_OF_BIN)[:4], by(G.STARVER)[:3], by(G.TWINS), by(123456789),
                             rng.choice(np.flatnonzero(groups < 0), 8, replace=False),
                             rng.choice(np.flatnonzero(groups >= 1000), 8, replace=False)])
    rows, bins = np.repeat(chosen, G.B), np.tile(np.arange(G.B), len(chosen))
    ctx.set_samples(X)
    dist, idx, nd, alpha = ctx.audit_pairs_witness(labels, G.B, m, rows, bins, groups=groups)
    cnt = check_padding(idx, nd, alpha)
    for k, r in enumerate(chosen):
        t_idx, t_dist, t_cnt = ctx.topm_per_bin(G.labels_without(labels, groups, r), G.B, m, np.array([r]))
        sl = slice(k * G.B, (k + 1) * G.B)
        assert np.array_equal(idx[sl], t_idx[0]) and np.array_equal(bits(nd[sl]), bits(t_dist[0])), r
        assert np.array_equal(cnt[sl], t_cnt[0])
        assert not np.isin(idx[sl][idx[sl] >= 0], G.withheld(groups, r)).any()
    # the groups with a purpose: bin 3 is gone for its own group, bin 2 is left with three members
    k = len(by(G.BIG)[:6])
    assert np.all(cnt[k * G.B + G.SMALL_BIN:(k + 4) * G.B:G.B] == 0) and np.all(dist[k * G.B + G.SMALL_BIN:(k + 4) * G.B:G.B] == np.inf)
    assert np.all(cnt[(k + 4) * G.B + G.STARVED_BIN:(k + 7) * G.B:G.B] == 3)


@pytest.mark.parametrize("name", ["base", "wide_d300"])
def test_lists_recruit_are_the_references_sets(ctx, name):
    c = CASES[name]
    B, m = c["B"], c["m"]
    X, labels, Y, row_of, bins, src = recruit_data(name)
    ref = recruit_reference(name)
    ctx.set_samples(X)
    dist, idx, nd, alpha = ctx.recruit_pairs_witness(labels, B, m, Y, row_of, bins)
    cnt = check_padding(idx, nd, alpha)
    for p in range(len(row_of)):
        want = ref.sets[row_of[p]][bins[p]]
        assert cnt[p] == len(want) and np.array_equal(idx[p, :cnt[p]], want), p
    # a copy of a labelled sample has that sample as its first vertex, at distance 0: nothing is withheld
    copies = np.flatnonzero((row_of >= 48) & (labels[src[row_of]] == bins))
    assert len(copies) >= 4
    assert np.all(nd[copies, 0] == 0.0) and np.all(X[idx[copies, 0]] == Y[row_of[copies]]) and np.all(dist[copies] == 0.0)
    # the distances are the selection arithmetic's: sqrt of the k-sequential unfused sum of squares
    real = idx >= 0
    diff = Y[row_of][:, None, :] - X[np.where(real, idx, 0)]
    acc = np.zeros(idx.shape)
    for k in range(X.shape[1]):
        acc = acc + diff[:, :, k] * diff[:, :, k]
    assert np.array_equal(bits(nd[real]), bits(np.sqrt(acc)[real]))


# ---- 3. the weights reproduce the distance

def reconstruction_ratio(X, y, dist, idx, nd, alpha):
    """(|| alpha @ X[nbr] - y || - dist) / bound per pair with vertices, test_gpu_parity.py:149-151's rule with scale =
    the pair's largest selection distance"""
    real = idx >= 0
    has = real.any(axis=1)
    point = np.einsum("pa,pad->pd", np.where(real, alpha, 0.0), X[np.where(real, idx, 0)])
    recon = np.linalg.norm(point - y, axis=1)
    scale = np.where(real, nd, 0.0).max(axis=1)
    bound = QP_TOL + 1e-7 * scale * (dist < 1e-6 * scale)
    return (np.abs(recon - dist) / bound)[has]


@pytest.mark.parametrize("name", list(CASES))
def test_weights_reproduce_the_distance(ctx, name):
    """Feasible weights whose combination lies at the returned distance; prints the case's worst ratio to the bound."""
    c = CASES[name]
    X, labels, _ = case_data(name)
    w = case_witness(ctx, name)
    dist, idx, nd, alpha = w["w"]
    real = idx >= 0
    has = real.any(axis=1)
    s = alpha.sum(axis=1)
    assert np.all(alpha[~real] == 0.0)
    assert np.all(np.abs(s[has] - 1.0) < 1e-12) and np.all(s[~has] == 0.0)
    if c.get("metric", "convex") == "convex":
        assert np.all(alpha >= 0.0)
    else:
        assert (alpha < 0.0).any()   # (the affine hull's nearest point need not lie between the vertices)
    ratio = reconstruction_ratio(X, X[w["rows"]], dist, idx, nd, alpha)
    print(f"{name}: worst |reconstruction - dist| / bound over {len(ratio)} pairs = {ratio.max():.3e}")
    assert ratio.max() <= 1.0


def test_weights_reproduce_the_distance_grouped_and_recruit(ctx):
    X, labels, groups = G.group_data()
    rows, bins = np.repeat(np.arange(0, G.N, 3), G.B), np.tile(np.arange(G.B), len(range(0, G.N, 3)))
    ctx.set_samples(X)
    dist, idx, nd, alpha = ctx.audit_pairs_witness(labels, G.B, 5, rows, bins, groups=groups)
    ratio = reconstruction_ratio(X, X[rows], dist, idx, nd, alpha)
    print(f"grouped: worst ratio over {len(ratio)} pairs = {ratio.max():.3e}")
    assert ratio.max() <= 1.0 and np.all(alpha >= 0.0)
    for name in ("base", "wide_d300"):
        c = CASES[name]
        X, labels, Y, row_of, bins, _ = recruit_data(name)
        ctx.set_samples(X)
        dist, idx, nd, alpha = ctx.recruit_pairs_witness(labels, c["B"], c["m"], Y, row_of, bins)
        assert np.all(np.abs(alpha.sum(axis=1) - 1.0) < 1e-12) and np.all(alpha >= 0.0)
        ratio = reconstruction_ratio(X, Y[row_of], dist, idx, nd, alpha)
        print(f"recruit {name}: worst ratio over {len(ratio)} pairs = {ratio.max():.3e}")
        assert ratio.max() <= 1.0


# ---- 4. tile and chunk edges, through the raw ABI (outputs longer than the call may write)

def ptr(a):
    return None if a is None else a.ctypes.data


def raw_audit(ctx, labels, groups, B, m, rows, bins, P, dist, idx, nd, alpha):
    return ctx._lib.chb_audit_pairs_witness(ctx._h, ptr(labels), ptr(groups), B, m, ptr(rows), ptr(bins), P,
                                            ptr(dist), ptr(idx), ptr(nd), ptr(alpha))


def raw_recruit(ctx, labels, B, m, Y, Q, D, row_of, bins, P, dist, idx, nd, alpha):
    return ctx._lib.chb_recruit_pairs_witness(ctx._h, ptr(labels), B, m, ptr(Y), Q, D, ptr(row_of), ptr(bins), P,
                                              ptr(dist), ptr(idx), ptr(nd), ptr(alpha))


def outputs(P, m, extra=5):
    """sentinel-filled outputs with room for `extra` pairs beyond P"""
    return (np.full(P + extra, -5.0), np.full((P + extra) * m, -55, dtype=np.int64), np.full((P + extra) * m, -5.0),
            np.full((P + extra) * m, -5.0))


def untouched(out, P, m):
    return all(np.all(a[(P if k == 0 else P * m):] == (-55 if a.dtype == np.int64 else -5.0)) for k, a in enumerate(out))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_tile_edges_of_one_bin(ctx, P):
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("base")
    w = case_witness(ctx, "base")
    ctx.set_samples(X)
    rows = np.ascontiguousarray(np.random.default_rng(40 + P).integers(0, len(X), P))
    bins = np.full(P, 2, dtype=np.int64)
    out = outputs(P, m)
    assert raw_audit(ctx, labels, None, B, m, rows, bins, P, *out) == 0
    assert untouched(out, P, m)   # a tile's tail rows score nothing and write nothing
    assert ctx.counter("pair_tiles") == (P + 63) // 64
    t_idx, t_dist, _ = w["topm"]
    assert np.array_equal(bits(out[0][:P]), bits(ctx.audit_pairs(labels, B, m, rows, bins)))
    assert np.array_equal(out[1][:P * m].reshape(P, m), t_idx[rows, 2])
    assert np.array_equal(bits(out[2][:P * m].reshape(P, m)), bits(t_dist[rows, 2]))
    ratio = reconstruction_ratio(X, X[rows], out[0][:P], out[1][:P * m].reshape(P, m), out[2][:P * m].reshape(P, m),
                                 out[3][:P * m].reshape(P, m))
    assert ratio.max() <= 1.0


def test_two_chunks(ctx):
    chunk = ctx.counter("recruit_chunk")
    assert chunk == 16384
    c = CASES["small_and_empty_bins"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("small_and_empty_bins")
    N = len(X)
    w = case_witness(ctx, "small_and_empty_bins")
    ctx.set_samples(X)
    P = chunk + 70
    p = np.arange(P)
    rows, bins = np.ascontiguousarray(p % N), np.ascontiguousarray((p // 7) % B)
    per = np.bincount(bins, minlength=B)
    assert per[:B - 1].sum() < chunk < per.sum() and len(np.unique(rows * B + bins)) < P   # the last bin's run straddles the cut
    out = outputs(P, m)
    ctx.profile_enable(True)
    ctx.profile_reset()
    assert raw_audit(ctx, labels, None, B, m, rows, bins, P, *out) == 0
    prof = ctx.profile_get("audit_pairs")
    ctx.profile_enable(False)
    assert prof["launches"] == 2 and prof["work"] == P   # one launch per chunk, under the plain call's name
    assert untouched(out, P, m)
    got = (out[0][:P], out[1][:P * m].reshape(P, m), out[2][:P * m].reshape(P, m), out[3][:P * m].reshape(P, m))
    assert np.array_equal(bits(got[0]), bits(ctx.audit_pairs(labels, B, m, rows, bins)))
    t_idx, t_dist, _ = w["topm"]   # (over every row of the case)
    assert np.array_equal(got[1], t_idx[rows, bins]) and np.array_equal(bits(got[2]), bits(t_dist[rows, bins]))
    key = rows * B + bins
    _, first = np.unique(key, return_index=True)
    first_of = dict(zip(key[first].tolist(), first.tolist()))
    rep = np.array([first_of[k] for k in key.tolist()])
    assert same(got, tuple(a[rep] for a in got))   # every repeat = its first occurrence, in all four outputs


def test_recruit_two_chunks(ctx):
    c = CASES["base"]
    B, m = c["B"], c["m"]
    X, labels, Y, _, _, _ = recruit_data("base")
    Y = np.ascontiguousarray(Y[:40])
    P = ctx.counter("recruit_chunk") + 70
    p = np.arange(P)
    row_of, bins = np.ascontiguousarray(p % 40), np.ascontiguousarray((p // 3) % B)
    ctx.set_samples(X)
    got = ctx.recruit_pairs_witness(labels, B, m, Y, row_of, bins)
    assert np.array_equal(bits(got[0]), bits(ctx.recruit_pairs(labels, B, m, Y, row_of, bins)))
    key = row_of * B + bins
    _, first = np.unique(key, return_index=True)
    first_of = dict(zip(key[first].tolist(), first.tolist()))
    rep = np.array([first_of[k] for k in key.tolist()])
    assert same(got, tuple(a[rep] for a in got))
    ref = recruit_reference("base")
    for q in range(P - 200, P):   # the second chunk's records, at the caller's positions
        want = ref.sets[row_of[q]][bins[q]]
        assert np.array_equal(got[1][q, :len(want)], want) and np.all(got[1][q, len(want):] == -1)


# ---- 5. optional outputs

def test_optional_outputs(ctx):
    c = CASES["m15"]
    B, m = c["B"], c["m"]
    X, labels, _ = case_data("m15")
    w = case_witness(ctx, "m15")
    P = 300
    rows, bins = np.ascontiguousarray(w["rows"][:P]), np.ascontiguousarray(w["bins"][:P])
    full = tuple(a[:P].reshape(-1) for a in w["w"])
    ctx.set_samples(X)
    for mask in range(1, 16):
        if (mask & 14) == 0:   # all three witness outputs null: refused (test_abi_refusals)
            continue
        out = outputs(P, m)
        args = [o if mask >> k & 1 else None for k, o in enumerate(out)]
        assert raw_audit(ctx, labels, None, B, m, rows, bins, P, *args) == 0, mask
        for k, o in enumerate(out):
            n = P if k == 0 else P * m
            if mask >> k & 1:
                assert same((o[:n],), (full[k],)), (mask, k)
            assert untouched(out, P, m)
    Xr, lr, Y, row_of, rbins, _ = recruit_data("base")
    cb = CASES["base"]
    ctx.set_samples(Xr)
    full = ctx.recruit_pairs_witness(lr, cb["B"], cb["m"], Y, row_of, rbins)
    P = len(row_of)
    for mask in (2, 4, 8, 6, 10, 12, 14):   # dist_out NULL with any of the others
        out = outputs(P, cb["m"])
        args = [o if mask >> k & 1 else None for k, o in enumerate(out)]
        assert raw_recruit(ctx, lr, cb["B"], cb["m"], Y, len(Y), Y.shape[1], row_of, rbins, P, *args) == 0, mask
        for k, o in enumerate(out):
            n = P if k == 0 else P * cb["m"]
            if mask >> k & 1:
                assert same((o[:n],), (full[k].reshape(-1),)), (mask, k)


# ---- 6. refusals

def test_abi_refusals():
    import test_gpu_recruit as R
    from chbin_amd import _lib, synth
    c = R.CASES["base"]
    X, labels, Y = R.case_data("base")
    N, D, B, m, Q = c["N"], c["D"], c["B"], c["m"], c["Q"]
    rng = np.random.default_rng(35)
    P = 90
    rows, row_of, bins = rng.integers(0, N, P), rng.integers(0, Q, P), rng.integers(0, B, P)
    groups = np.arange(N, dtype=np.int64) // 3
    out = outputs(P, 17, extra=0)
    ctx = _lib.Context(0)
    other = _lib.Context(0)
    try:
        lib = ctx._lib
        A = lambda *a: raw_audit(ctx, *a)
        Rc = lambda *a: raw_recruit(ctx, *a)
        # no samples
        assert A(labels, None, B, m, rows, bins, P, *out) == ESTATE
        assert Rc(labels, B, m, Y, Q, D, row_of, bins, P, *out) == ESTATE
        ctx.set_samples(X)
        ref_a = ctx.audit_pairs_witness(labels, B, m, rows, bins)
        ref_r = ctx.recruit_pairs_witness(labels, B, m, Y, row_of, bins)
        tiles = ctx.counter("pair_tiles")

        def refused(rc, code, text=None):
            assert rc == code, (rc, code, lib.chb_last_error())
            assert untouched(out, 0, 17)                   # nothing was written
            assert ctx.counter("pair_tiles") == tiles      # ... or counted
            if text is not None:
                assert text in lib.chb_last_error(), lib.chb_last_error()

        # no witness output at all
        refused(A(labels, None, B, m, rows, bins, P, out[0], None, None, None), EINVAL, b"without witnesses")
        refused(A(labels, groups, B, m, rows, bins, P, out[0], None, None, None), EINVAL, b"without witnesses")
        refused(Rc(labels, B, m, Y, Q, D, row_of, bins, P, out[0], None, None, None), EINVAL, b"without witnesses")
        # limits
        for g in (None, groups):
            refused(A(labels, g, B, 17, rows, bins, P, *out), EUNSUPPORTED, b"16")
            refused(A(labels, g, 8193, m, rows, bins, P, *out), EUNSUPPORTED, b"8192")
        refused(Rc(labels, B, 17, Y, Q, D, row_of, bins, P, *out), EUNSUPPORTED, b"16")
        refused(Rc(labels, 8193, m, Y, Q, D, row_of, bins, P, *out), EUNSUPPORTED, b"8192")
        # an entry out of range in each index array
        for bad in (-1, B):
            b2 = bins.copy()
            b2[P // 2] = bad
            refused(A(labels, None, B, m, rows, b2, P, *out), EINVAL, b"bin_idx")
            refused(A(labels, groups, B, m, rows, b2, P, *out), EINVAL, b"bin_idx")
            refused(Rc(labels, B, m, Y, Q, D, row_of, b2, P, *out), EINVAL, b"bin_idx")
        for bad in (-1, N):
            r2 = rows.copy()
            r2[P - 1] = bad
            refused(A(labels, None, B, m, r2, bins, P, *out), EINVAL, b"row_idx")
        for bad in (-1, Q):
            r2 = row_of.copy()
            r2[0] = bad
            refused(Rc(labels, B, m, Y, Q, D, r2, bins, P, *out), EINVAL, b"row_of")
        # D, null arguments, ranges
        refused(Rc(labels, B, m, Y, Q, D - 1, row_of, bins, P, *out), EINVAL)
        refused(Rc(labels, B, m, Y, Q, D + 1, row_of, bins, P, *out), EINVAL)
        refused(A(None, None, B, m, rows, bins, P, *out), EINVAL)
        refused(A(labels, None, B, m, None, bins, P, *out), EINVAL)
        refused(A(labels, None, B, m, rows, None, P, *out), EINVAL)
        refused(Rc(labels, B, m, None, Q, D, row_of, bins, P, *out), EINVAL)
        refused(Rc(labels, B, m, Y, Q, D, None, bins, P, *out), EINVAL)
        refused(A(labels, None, B, m, rows, bins, -1, *out), EINVAL)
        refused(A(labels, None, 0, m, rows, bins, P, *out), EINVAL)
        refused(A(labels, None, B, 0, rows, bins, P, *out), EINVAL)
        # P = 0: CHB_OK, nothing is read, written or counted
        refused(A(None, None, B, m, None, None, 0, None, None, None, None), 0)
        refused(A(labels, groups, B, m, rows, bins, 0, *out), 0)
        refused(Rc(None, B, m, None, 0, D, None, None, 0, None, None, None, None), 0)
        refused(Rc(labels, B, m, Y, Q, D, row_of, bins, 0, *out), 0)
        empty = ctx.audit_pairs_witness(labels, B, m, [], [])
        assert empty[0].shape == (0,) and empty[1].shape == (0, m)
        # the context still answers, with the same bits
        assert same(ctx.audit_pairs_witness(labels, B, m, rows, bins), ref_a)
        assert same(ctx.recruit_pairs_witness(labels, B, m, Y, row_of, bins), ref_r)
        tiles = ctx.counter("pair_tiles")

        # ---- an open stepwise fit: refused, and the fit completes with the labels it gives without the calls
        _, initial, _ = synth.make_synthetic(N + Q, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
        initial = initial[:N].copy()
        sl = np.random.default_rng(5).permutation(np.flatnonzero(initial == -1))[:200].astype(np.int64)
        other.set_samples(X)
        res = {}
        for who, cx in (("disturbed", ctx), ("plain", other)):
            cx.fit_begin(B, initial, m)
            if who == "disturbed":
                refused(A(labels, None, B, m, rows, bins, P, *out), ESTATE)
            cx.batch_begin(sl, 0, len(sl))
            guess = np.full(len(sl), -1, dtype=np.int64)
            cx.batch_guess(guess)
            lab1, md1 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(guess, 0, lab1, md1)
            if who == "disturbed":
                refused(A(labels, groups, B, m, rows, bins, P, *out), ESTATE)
                refused(Rc(labels, B, m, Y, Q, D, row_of, bins, P, *out), ESTATE)
            lab2, md2 = np.full(len(sl), -9, dtype=np.int64), np.zeros(len(sl))
            cx.batch_round(lab1, 0, lab2, md2)
            cx.batch_commit(lab2)
            res[who] = (lab1, lab2, cx.fit_labels())
        for a, b in zip(res["disturbed"], res["plain"]):
            assert np.array_equal(a, b)
        assert np.all(res["plain"][1] >= 0)
        ctx.set_samples(X)   # ends the stepwise fit
        assert same(ctx.audit_pairs_witness(labels, B, m, rows, bins), ref_a)
    finally:
        ctx.close()
        other.close()


# ---- 7. no trace in a fit

def test_no_trace_left_in_a_fit():
    """fit_cluster, the witness calls, the same fit again on one context: labels, sweeps and change counts identical, every
    counter but "pair_tiles" and the fit statistics as without the calls in between."""
    from chbin_amd import _lib, synth
    from test_gpu_pairs import COUNTERS, tiles_of
    N, D, B, m, its = 2500, 136, 8, 5, 3
    Z, initial, _ = synth.make_synthetic(N + 200, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    initial = initial[:N].copy()
    perms = synth.draw_permutations(initial, its, seed=0)
    rng = np.random.default_rng(36)
    row_of, ybins = rng.integers(0, len(Y), 500), rng.integers(0, B, 500)
    groups = np.arange(N, dtype=np.int64) // 2

    def two_fits(calls_between):
        ctx = _lib.Context(0)
        try:
            ctx.set_samples(X)
            res = []
            for k in range(2):
                lab, sweeps, changed = ctx.fit_cluster(B, initial, perms, m, its)
                res.append((lab, sweeps, changed, [ctx.counter(n) for n in COUNTERS], ctx.fit_stats()))
                if k == 0 and calls_between:
                    assert ctx.counter("pair_tiles") == 0 and np.all((lab >= 0) & (lab < B))
                    own = ctx.audit_pairs_witness(lab, B, m, np.arange(N), lab)
                    assert np.isfinite(own[0]).all() and np.all(own[1] >= 0)
                    assert ctx.counter("pair_tiles") == tiles_of(lab, B)
                    assert np.isfinite(ctx.audit_pairs_witness(lab, B, m, np.arange(N), lab, groups=groups)[0]).all()
                    assert np.isfinite(ctx.recruit_pairs_witness(lab, B, m, Y, row_of, ybins)[0]).all()
                    assert ctx.counter("pair_tiles") == tiles_of(ybins, B)
                    assert [ctx.counter(n) for n in COUNTERS] == res[0][3]
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


# ---- 8. the Python mirror

@pytest.mark.parametrize("name", ["small_and_empty_bins", "affine"])
def test_mirror_functions(ctx, name):
    from chbin_amd import _lib, clustering
    c = CASES[name]
    B, m, metric = c["B"], c["m"], c.get("metric", "convex")
    X, labels, _ = case_data(name)
    D = X.shape[1]
    w = case_witness(ctx, name)
    rows, bins = w["rows"][:500], w["bins"][:500]
    got = clustering.witness(X, labels, rows, bins, B, num_neighbors=m, metric=metric)
    assert isinstance(got, clustering.Witness)
    assert same((got.dist, got.neighbors, got.neighbor_dist, got.weights), tuple(a[:500] for a in w["w"]))
    assert _lib.default_context().get_metric() == "convex"
    real = got.neighbors >= 0
    assert np.array_equal(got.count, real.sum(axis=1))
    if name == "small_and_empty_bins":
        assert {0, 1, 2, m} <= set(got.count.tolist())   # padded pairs among them
    assert got.support.shape == (500, m) and not got.support[~real].any()
    point = got.nearest_point(X)
    assert point.shape == (500, D) and np.isfinite(point).all()
    blocks = [(0, 10), (10, D - 3), (D - 3, D)]   # a partition of the columns
    res = got.residual_by_block(X, X[rows], blocks)
    assert res.shape == (500, 3)
    has = got.count > 0
    assert np.isnan(res[~has]).all() and np.all(res[has] >= 0.0)
    # the blocks' sum is dist**2 within item 3's bound in squared form: |r^2 - d^2| = |r - d| (r + d) <= b (2 d + b)
    scale = np.where(real, got.neighbor_dist, 0.0).max(axis=1)[has]
    d = got.dist[has]
    b = QP_TOL + 1e-7 * scale * (d < 1e-6 * scale)
    assert np.all(np.abs(res[has].sum(axis=1) - d ** 2) <= b * (2.0 * d + b))
    # grouped, and the recruit form
    Xg, lg, groups = G.group_data()
    gr, gb = np.arange(0, G.N, 5), np.arange(0, G.N, 5) % G.B
    gw = clustering.witness(Xg, lg, gr, gb, G.B, num_neighbors=5, groups=groups)
    ctx.set_samples(Xg)
    assert same((gw.dist, gw.neighbors, gw.neighbor_dist, gw.weights),
                ctx.audit_pairs_witness(lg, G.B, 5, gr, gb, groups=groups))
    Xr, lr, Y, row_of, rbins, _ = recruit_data("base")
    cb = CASES["base"]
    rw = clustering.recruit_witness(Xr, lr, Y, row_of, rbins, cb["B"], num_neighbors=cb["m"])
    ctx.set_samples(Xr)
    assert same((rw.dist, rw.neighbors, rw.neighbor_dist, rw.weights),
                ctx.recruit_pairs_witness(lr, cb["B"], cb["m"], Y, row_of, rbins))
    assert rw.residual_by_block(Xr, Y[row_of], [(0, 136)]).shape == (len(row_of), 1)
