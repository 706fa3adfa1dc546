"""The bin-count axis, B = 9 .. 8192, on every entry point (include/chbin_hip.h promises each of them up to 8192 bins; the
other modules stop at 8 bins for row scoring, 7 for chb_topm_per_bin and 500 -- never against the oracle -- for fits).

References: the CPU oracle (oracle.sweep(..., want_all=True), oracle.fit_cluster, oracle.find_nearest_from_cluster,
oracle.cdist_row) and plain numpy; the library itself only where one call is defined by another (the bin report by the
audit, a _multi slice by the single-m call).  Tolerances are the project's: QP_TOL = 1e-9 absolute on finite hull
distances, the +inf pattern exactly, selection indices and cdist-style distances bit for bit, labels / sweeps / change
counts equal.

1. Row scoring (ROW_CASES; sigma=6e-3, mix=0.5, the generator's labels with about 30 % set to -1, Q rows at random), the
   reduce kernel's 8 lanes with several bins each, the report kernel's later bin tiles.  By the oracle alone (audit rows /
   recruit rows; "left out" = rows within 2 * QP_TOL of a tie, which check_against_oracle leaves out of the bin
   comparison -- its cap stays at 1 %):
     case    smallest oracle margin   rows left out   +inf entries   oracle, one CPU thread
     b9      3.3e-04 / 1.2e-05        0 / 0           none           0.2 s + 0.2 s
     b65     2.0e-05 / 3.5e-06        0 / 0           none           1.1 s + 1.1 s
     b200    8.2e-06 / 7.3e-06        0 / 0           none           3.2 s + 3.1 s
     b1100   7.4e-06 / 5.9e-05        0 / 0           2.1 %          8.7 s + 8.3 s
     b8192   4.6e-05 / 1.2e-04        0 / 0           36.3 %         7.4 s + 8.0 s
2. Exact ties between bins at B > 8, built by hand on the b200 data, against strict_scan over the call's own distances
   and, for the zero cases, the stated constants.
3. chb_topm_per_bin at B = 200 / 1100, across the 4096-query chunk of its host loop, and at m = 24 / 64 (the generic
   selection kernel), per (query, bin) against oracle.find_nearest_from_cluster.
4. Whole fits, one per shells-per-bin class of the CSR key (FIT_CASES; sigma=3e-3, mix=0.2), through the product library;
   the cases with B <= 1100 also through the developer library, every entry of the n_move x B matrix against the oracle.
   The larger cases are product-only (the developer dump is N x B doubles: 0.25 GB at b4100, 1 GB at b8192).
   The oracle's cost per visit is B hull problems (21 ms at b300, 25 ms at b600, 130 ms at b1100, 62 ms at b2100, 90 ms
   at b4100, 190 ms at b8192, one CPU thread), so N and the seeds per bin are set for a few hundred movable contigs and a
   replay below 30 s; every bin still starts with fewer than m members, except at b8192 (5912 of 8192 do).  Per case, one
   oracle replay on one CPU thread and the smallest margin of the last sweep's visits -- no visit of any case lies within
   4 * QP_TOL of a tie, so label equality is a fair demand:
     case    movable   empty bins   replay    smallest margin
     b300    358       4            15.2 s    4.2e-03
     b600    210       33           10.6 s    3.7e-03
     b1100   186       9            24.4 s    1.4e-02
     b2100   307       203          18.9 s    1.6e-02
     b4100   208       640          18.7 s    2.3e-02
     b8192   105       1289         20.2 s    1.9e-02
   And tile skipping below 32 shells per bin (B = 300, five coverage columns): test_tile_skipping_at_16_shells.
5. B = 8193 is CHB_EUNSUPPORTED from chb_fit_cluster, chb_topm_per_bin and chb_fit_begin (the row-scoring calls'
   refusals are in their own modules), and the context stays usable."""
import functools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_audit as audit_mod
import test_gpu_recruit as recruit_mod
from test_gpu_bin_distances import CHILD, COUNTERS, DEV_LIB, ROOT, _ctx_env, _margin, _min2, oracle_replay
from test_gpu_bin_report import check_report, expected
from test_gpu_recruit import QP_TOL, check_against_oracle, check_reduction, strict_scan

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -5

# ---------------------------------------------------------------------------------------------- 1. row scoring

# b9: one lane of the reduce kernel holds two bins; b65: a second bin tile of the report with 63 lanes past the last bin;
# b200: the benchmark's bin count; b1100: empty bins (+inf entries); b8192: the limit, most bins of one to three members
ROW_CASES = {
    "b9": dict(N=3000, D=64, B=9, m=5, Q=130, ms=(1, 3, 16)),
    "b65": dict(N=3000, D=64, B=65, m=5, Q=130, ms=(1, 3, 16)),
    "b200": dict(N=4000, D=64, B=200, m=5, Q=130, ms=(1, 3, 16)),
    "b1100": dict(N=6000, D=32, B=1100, m=5, Q=130, ms=(1, 3, 16)),
    "b8192": dict(N=12000, D=16, B=8192, m=3, Q=70, ms=(1, 3)),
}
ROW_NAMES = list(ROW_CASES)


@functools.lru_cache(maxsize=None)
def row_data(name):
    """(X, labels, rows, Y) of a case; deterministic.  rows = Q resident rows chosen at random, Y = Q fresh rows."""
    from chbin_amd import synth
    c = ROW_CASES[name]
    N, D, B, Q = c["N"], c["D"], c["B"], c["Q"]
    Z, _, true = synth.make_synthetic(N + Q, D, B, seed=N + D + B + c["m"], sigma=6e-3, mix=0.5)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    rng = np.random.default_rng(7)
    labels = true[:N].copy()
    labels[rng.random(N) < 0.3] = -1
    rows = np.sort(rng.choice(N, Q, replace=False)).astype(np.int64)
    for a in (X, Y, labels, rows):
        a.setflags(write=False)
    return X, labels, rows, Y


def row_oracle(name, kind):
    c = ROW_CASES[name]
    X, labels, rows, Y = row_data(name)
    if kind == "audit":
        d = audit_mod.oracle_rows(X, labels, rows, c["B"], c["m"])
    else:
        d = recruit_mod.oracle_rows(X, labels, Y, c["B"], c["m"])
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def oracles():
    """Every oracle answer of the module, on up to 8 threads (the oracle is a ctypes library: each call drops the GIL)
    while the GPU tests go on.  {key: future}."""
    pool = ThreadPoolExecutor(max_workers=8)
    out = {}
    # (the slowest first)
    for name in sorted(FIT_CASES, key=lambda n: -FIT_CASES[n]["B"]):
        out["fit", name] = pool.submit(fit_oracle, name)
    for name in reversed(ROW_NAMES):
        for kind in ("audit", "recruit"):
            out[name, kind] = pool.submit(row_oracle, name, kind)
    yield out
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _bits_equal(a, b):
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


@pytest.mark.parametrize("name", ROW_NAMES)
def test_audit_and_recruit_match_oracle(ctx, oracles, name):
    c = ROW_CASES[name]
    B, m = c["B"], c["m"]
    X, labels, rows, Y = row_data(name)
    ctx.set_samples(X)
    for kind, got in (("audit", ctx.audit_rows(labels, B, m, rows)), ("recruit", ctx.recruit_rows(labels, B, m, Y))):
        bins, dist, mind, margin = got
        assert dist.shape == (c["Q"], B)
        check_reduction(bins, dist, mind, margin)
        want = oracles[name, kind].result()
        check_against_oracle(f"{name}/{kind}", bins, dist, want)
        print(f"{name}/{kind}: {np.isinf(want).mean():.1%} of the entries +inf")
    sizes = np.bincount(labels[labels >= 0], minlength=B)
    if name == "b1100":
        assert (sizes == 0).any() and ((sizes > 0) & (sizes < m)).any()
    if name == "b8192":
        assert sizes.max() <= 6 and (sizes == 0).mean() > 0.3


@pytest.mark.parametrize("name", ROW_NAMES)
def test_multi_slices_are_the_single_m_calls(ctx, name):
    c = ROW_CASES[name]
    B, ms = c["B"], c["ms"]
    X, labels, rows, Y = row_data(name)
    ctx.set_samples(X)
    multi_a = ctx.audit_rows_multi(labels, B, ms, rows)
    multi_r = ctx.recruit_rows_multi(labels, B, ms, Y)
    for j, m in enumerate(ms):
        for multi, single in ((multi_a, ctx.audit_rows(labels, B, m, rows)), (multi_r, ctx.recruit_rows(labels, B, m, Y))):
            for a, b in zip(multi, single):
                assert a[j].shape == b.shape and _bits_equal(np.ascontiguousarray(a[j]), b), (name, m)
            check_reduction(single[0], single[1], single[2], single[3])


def dsum_block_order(labels, B, rows, dist):
    """dsum as include/chbin_hip.h guarantees it: a label's rows in the call's order, in blocks of 64, each block summed in
    order from 0, the block sums added in order from 0."""
    own = labels[rows]
    want = np.zeros((B, B))
    for a in np.unique(own[(own >= 0) & (own < B)]):
        d = dist[own == a]
        fin = np.isfinite(d)
        total = np.zeros(B)
        for r0 in range(0, len(d), 64):
            s = np.zeros(B)
            for k in range(r0, min(r0 + 64, len(d))):   # (x + 0.0 == x bit for bit for the finite, non-negative x here)
                s = s + np.where(fin[k], d[k], 0.0)
            total = total + s
        want[a] = total
    return want


@pytest.mark.parametrize("name", [n for n in ROW_NAMES if n != "b8192"])
def test_bin_report_matches_the_audit(ctx, name):
    c = ROW_CASES[name]
    B, m = c["B"], c["m"]
    X, labels, rows, _ = row_data(name)
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
    got = ctx.bin_report(labels, B, m, rows)
    want = expected(labels, B, rows, bins, dist)
    check_report(name, got, want)
    assert _bits_equal(got[4], dsum_block_order(labels, B, rows, dist)), name
    assert got[0].sum() + got[1].sum() + got[5] == len(rows) and got[5] > 0
    if B > 64:   # rows whose own label lies in a later bin tile, and cells in one
        assert (labels[rows] >= 64).any() and got[2][:64, 64:].any() and got[2][64:, 64:].any()
    if name == "b1100":   # only unplaced and confusion requested
        lib = ctx._lib
        conf, unplaced = np.full((B, B), -5, dtype=np.int64), np.full(B, -5, dtype=np.int64)
        rc = lib.chb_bin_report(ctx._h, labels.ctypes.data, B, m, rows.ctypes.data, len(rows), conf.ctypes.data,
                                unplaced.ctypes.data, None, None, None, None)
        assert rc == 0 and np.array_equal(conf, want[0]) and np.array_equal(unplaced, want[1])


@pytest.mark.parametrize("own", [63, 64, 199])
def test_bin_report_unplaced_row_of_a_later_tile(ctx, own):
    """unplaced is written by the first bin tile's workgroup alone.  A row chooses no bin only if no other sample carries a
    label: one labelled row per call, its label in the first tile's last lane, a later tile's first and the last bin."""
    B, m = 200, 5
    X, _, rows, _ = row_data("b200")
    labels = np.full(len(X), -1, dtype=np.int64)
    labels[rows[5]] = own
    ctx.set_samples(X)
    bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
    assert bins[5] == -1 and np.all(np.isinf(dist[5]))
    got = ctx.bin_report(labels, B, m, rows)
    check_report(f"unplaced_{own}", got, expected(labels, B, rows, bins, dist))
    want = np.zeros(B, dtype=np.int64)
    want[own] = 1
    assert np.array_equal(got[1], want) and got[0].sum() == 0 and got[2].sum() == 0 and got[5] == len(rows) - 1


# ---------------------------------------------------------------------------------------------- 2. exact ties

def _free_rows(labels, taken, n):
    """n unlabelled sample indices, ascending, none of them in `taken`"""
    free = np.setdiff1d(np.flatnonzero(labels == -1), np.asarray(sorted(taken), dtype=np.int64))
    assert len(free) >= n
    return free[:n]


def _with_twins(twin_bins):
    """The b200 data with one unlabelled sample s given twins (rows copied bit for bit) labelled `twin_bins`.
    Returns (X, labels, s, Y): Y's first row is a copy of s, the others are the case's own."""
    X0, labels0, rows, Y0 = row_data("b200")
    X, labels, Y = X0.copy(), labels0.copy(), Y0.copy()
    s = int(np.flatnonzero(labels == -1)[17])
    twins = _free_rows(labels, {s} | set(rows.tolist()), len(twin_bins))
    X[twins] = X[s]
    labels[twins] = twin_bins
    Y[0] = X[s]
    return X, labels, s, Y


# lane of the reduce kernel = bin % 8: 3, 11 and 19 share lane 3; 5 sits in lane 5, 12 in lane 4
@pytest.mark.parametrize("twin_bins,lowest", [((3, 11, 19, 5, 12), 3),   # all five
                                              ((11, 19, 12), 11),        # lane 3 meets bin 3 first, which is not tied
                                              ((12, 5), 5),              # between lanes only (the lower bin in the higher lane)
                                              ((19, 11), 11)],           # within one lane only
                         ids=["five", "not_first_in_lane", "cross_lane_only", "in_lane_only"])
def test_exact_zero_ties(ctx, twin_bins, lowest):
    B, m = 200, 5
    assert {b % 8 for b in (3, 11, 19)} == {3} and 5 % 8 != 12 % 8
    X, labels, s, Y = _with_twins(twin_bins)
    ctx.set_samples(X)
    rows = np.array([s, s + 1, s], dtype=np.int64)
    for what, (bins, dist, mind, margin) in (("audit", ctx.audit_rows(labels, B, m, rows)),
                                             ("recruit", ctx.recruit_rows(labels, B, m, Y))):
        check_reduction(bins, dist, mind, margin)
        zero = np.flatnonzero(dist[0] == 0.0)
        assert sorted(zero.tolist()) == sorted(twin_bins), (what, zero)
        assert bins[0] == lowest and mind[0] == 0.0 and margin[0] == 0.0, (what, bins[0], mind[0], margin[0])
        assert not np.signbit(mind[0]) and not np.signbit(margin[0])


@pytest.mark.parametrize("a,b", [(24, 40), (52, 30)], ids=["same_lane", "other_lanes"])
def test_nonzero_tie_between_identical_bins(ctx, a, b):
    """Bin b gets bin a's member set through duplicated rows (in the same index order, so the (distance, index) order of
    the selection is the same too): the two hulls are bitwise the same problem, the tied minimum of a row near them is not
    zero.  (24 and 52 are large bins of the case: by the oracle the six rows taken out of either still choose it.)"""
    B, m = 200, 5
    assert (a % 8 == b % 8) == (a == 24)
    X0, labels0, _, Y0 = row_data("b200")
    X, labels = X0.copy(), labels0.copy()
    labels[labels == b] = -1
    near = np.flatnonzero(labels == a)[-6:]   # six of bin a's own members, taken out of it: the rows to score
    labels[near] = -1
    mem_a = np.flatnonzero(labels == a)
    assert len(mem_a) >= m
    copies = _free_rows(labels, set(near.tolist()), len(mem_a))
    X[copies] = X[mem_a]
    labels[copies] = b
    ctx.set_samples(X)
    Y = np.vstack([X[near], Y0[:10]])   # (an unlabelled resident row is as new to the bins as any other row)
    for what, (bins, dist, mind, margin) in (("audit", ctx.audit_rows(labels, B, m, near.astype(np.int64))),
                                             ("recruit", ctx.recruit_rows(labels, B, m, Y))):
        check_reduction(bins, dist, mind, margin)
        assert _bits_equal(np.ascontiguousarray(dist[:, a]), np.ascontiguousarray(dist[:, b])), what
        tied = dist[:, a] == dist.min(axis=1)
        assert tied.sum() >= 3, (what, tied.sum())
        assert np.all(bins[tied] == min(a, b)) and np.all(margin[tied] == 0.0) and np.all(mind[tied] > 0.0), what


@pytest.mark.parametrize("keep", [(15,), (6, 22), (199,), (7, 8)], ids=["one_high_lane", "two_same_lane", "last_bin", "two_lanes"])
def test_rows_with_one_or_two_finite_bins(ctx, keep):
    """Every bin +inf except one in a high lane (bin 15: lane 7; bin 199: lane 7, the last bin): that bin, margin +inf.
    Exactly two finite bins, in the same lane (6 and 22) and in neighbouring lanes."""
    B, m = 200, 5
    X, labels0, rows, Y = row_data("b200")
    labels = np.where(np.isin(labels0, keep), labels0, -1)
    ctx.set_samples(X)
    for bins, dist, mind, margin in (ctx.audit_rows(labels, B, m, rows), ctx.recruit_rows(labels, B, m, Y)):
        check_reduction(bins, dist, mind, margin)
        fin = np.isfinite(dist)
        assert np.array_equal(np.flatnonzero(fin.all(axis=0)), np.sort(keep)) and fin.sum() == len(keep) * len(dist)
        if len(keep) == 1:
            assert np.all(bins == keep[0]) and np.all(margin == np.inf) and np.array_equal(mind, dist[:, keep[0]])
        else:
            lo, hi = dist[:, keep].min(axis=1), dist[:, keep].max(axis=1)
            assert np.array_equal(mind, lo) and np.array_equal(margin, hi - lo)
            assert len(set(bins.tolist())) == 2   # (each of the two wins somewhere)


# ---------------------------------------------------------------------------------------------- 3. chb_topm_per_bin

def check_topm(X, labels, B, m, queries, got, check=None):
    """idx / dist / cnt of chb_topm_per_bin against oracle.find_nearest_from_cluster per (query, bin), for the positions
    `check` of `queries` (all of them by default).  The oracle's list is ordered by (distance, index)."""
    from oracle import oracle as O
    idx, dist, cnt = got
    assert idx.shape == (len(queries), B, m) and dist.shape == idx.shape and cnt.shape == (len(queries), B)
    for qi in (range(len(queries)) if check is None else check):
        q = int(queries[qi])
        cur = labels.copy()
        cur[q] = -1
        row = O.cdist_row(X, q)
        for c in range(B):
            want = O.find_nearest_from_cluster(c, cur, row, m)
            n = cnt[qi, c]
            assert n == len(want), (q, c)
            assert np.array_equal(idx[qi, c, :n], want), (q, c)
            assert np.array_equal(dist[qi, c, :n], row[want]), (q, c)   # bit-exact distances
            assert np.all(idx[qi, c, n:] == -1)


@pytest.mark.parametrize("name,m,n_check", [("b200", 5, 150), ("b1100", 16, 40)])
def test_topm_per_bin_many_bins(ctx, name, m, n_check):
    c = ROW_CASES[name]
    B = c["B"]
    X0, labels, _, _ = row_data(name)
    X = X0.copy()
    rng = np.random.default_rng(B + m)
    X[10] = X[3]; X[11] = X[3]; X[500] = X[499]          # exact duplicates -> distance ties
    labels = labels.copy()
    labels[[3, 10, 11]] = 2
    queries = np.concatenate([rng.choice(len(X), 144, replace=False), [3, 10, 11, 499, 500, 3]]).astype(np.int64)
    assert len(queries) == 150
    ctx.set_samples(X)
    got = ctx.topm_per_bin(labels, B, m, queries)
    check = None if n_check == len(queries) else np.concatenate([np.arange(n_check - 6), np.arange(144, 150)])
    check_topm(X, labels, B, m, queries, got, check)
    sizes = np.bincount(labels[labels >= 0], minlength=B)
    assert got[2].max() == min(m, sizes.max())
    if name == "b1100":   # (no bin has 16 members: every list is short, some are empty)
        assert sizes.max() < m and got[2].min() == 0


def test_topm_per_bin_across_the_query_chunk(ctx):
    """4096 + 37 distinct queries and one repeat: the host loop's chunks are 4096, 37 and -- a chunk holds no sample twice
    -- the repeat alone.  Against the oracle on a random 200 positions, and bit for bit against the same queries asked
    in two separate calls."""
    from chbin_amd import synth
    N, D, B, m = 6000, 8, 9, 3
    X, _, true = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.5)
    rng = np.random.default_rng(7)
    labels = true.copy()
    labels[rng.random(N) < 0.3] = -1
    Q = 4096 + 37
    queries = rng.choice(N, Q, replace=False).astype(np.int64)
    queries = np.append(queries, queries[4096 + 20])
    ctx.set_samples(X)
    got = ctx.topm_per_bin(labels, B, m, queries)
    check = np.concatenate([rng.choice(Q, 194, replace=False), [4095, 4096, 4096 + 20, Q - 1, Q, 0]])
    check_topm(X, labels, B, m, queries, got, check)
    first = ctx.topm_per_bin(labels, B, m, queries[:2000])
    second = ctx.topm_per_bin(labels, B, m, queries[2000:])
    for g, a, b in zip(got, first, second):
        assert _bits_equal(g, np.concatenate([a, b]))
    for g in got:
        assert _bits_equal(g[Q], g[4096 + 20])


@pytest.mark.parametrize("m", [24, 64])
def test_topm_per_bin_generic_selection(ctx, m):
    """m > 16: chb_topm_per_bin runs the generic selection kernel.  The generic_m24 data of test_gpu_bin_distances.py (about
    85 labelled members per bin), one bin cut down to 20 members (fewer than either m)."""
    from chbin_amd import synth
    N, D, B = 360, 64, 3
    X, _, true = synth.make_synthetic(N, D, B, seed=N + D + B + 24, sigma=6e-3, mix=0.5, n_seed=30)
    rng = np.random.default_rng(m)
    labels = true.copy()
    labels[rng.random(N) < 0.25] = -1
    labels[np.flatnonzero(labels == 1)[20:]] = -1
    X[10] = X[3]; X[11] = X[3]
    labels[[3, 10, 11]] = 2
    queries = np.concatenate([rng.choice(N, 57, replace=False), [3, 10, 3]]).astype(np.int64)
    ctx.set_samples(X)
    got = ctx.topm_per_bin(labels, B, m, queries)
    check_topm(X, labels, B, m, queries, got)
    sizes = np.bincount(labels[labels >= 0], minlength=B)
    assert sizes[1] <= 20 < m and got[2][:, 1].max() == sizes[1] and got[2].max() == min(m, sizes.max())


# ---------------------------------------------------------------------------------------------- 4. whole fits

# name: N, D, B, m, sweeps, seeds per bin; nsh = the shells per bin of the CSR key that fit_begin_impl arrives at
FIT_CASES = {
    "b300": dict(N=1400, D=136, B=300, m=5, its=2, n_seed=4, nsh=16, dev=True),
    "b600": dict(N=1850, D=136, B=600, m=5, its=2, n_seed=4, nsh=8, dev=True),
    "b1100": dict(N=5000, D=64, B=1100, m=8, its=1, n_seed=7, nsh=4, dev=True),
    "b2100": dict(N=5000, D=64, B=2100, m=5, its=1, n_seed=4, nsh=2, dev=False),
    "b4100": dict(N=7500, D=32, B=4100, m=5, its=1, n_seed=4, nsh=1, dev=False),
    "b8192": dict(N=15000, D=16, B=8192, m=3, its=1, n_seed=5, nsh=1, dev=False),
}
FIT_NAMES = list(FIT_CASES)


def shells_per_bin(B):
    nsh = 32
    while nsh > 1 and B * nsh > 8192:
        nsh >>= 1
    return nsh


@functools.lru_cache(maxsize=None)
def fit_data(name):
    """(X, initial, perms) of a case; deterministic."""
    from chbin_amd import synth
    c = FIT_CASES[name]
    N, D, B = c["N"], c["D"], c["B"]
    X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + c["m"] + c.get("reseed", 0), sigma=3e-3, mix=0.2,
                                         n_seed=c["n_seed"])
    perms = synth.draw_permutations(initial, c["its"], seed=0)
    return np.ascontiguousarray(X), initial, perms


def fit_oracle(name):
    """oracle_replay without its dense N x B array (1.1 GB at b8192): (labels, sweeps, changes, the movable contigs in
    ascending order, their n_move x B distances of the last sweep)."""
    from oracle import oracle as O
    c = FIT_CASES[name]
    X, initial, perms = fit_data(name)
    B, m, its = c["B"], c["m"], c["its"]
    if B * len(X) <= 4_000_000:
        lab, its_o, ch, full = oracle_replay(X, B, initial, perms, m, its)
        mv = np.flatnonzero(initial < 0)
        return lab, its_o, ch, mv, full[mv]
    assert its == 1
    after, _, alld = O.sweep(X, B, initial, perms[0], m, want_all=True)
    order = np.argsort(perms[0])
    return after, 1, np.array([np.count_nonzero(after != initial)]), perms[0][order], alld[order]


@pytest.mark.parametrize("name", FIT_NAMES)
def test_fit_matches_oracle(oracles, name):
    """Product library: labels, sweeps and changes equal the oracle's; min_dist is the row minimum of the oracle's last
    sweep, margin second-smallest minus smallest; seeds are NaN; the fused path ran and no shortlist was short."""
    c = FIT_CASES[name]
    B = c["B"]
    assert shells_per_bin(B) == c["nsh"]
    X, initial, perms = fit_data(name)
    from chbin_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_samples(X)
        lab, its, ch, mind, margin = ctx.fit_cluster_margins(B, initial, perms, c["m"], c["its"], want_min_dist=True)
        cnt = {k: ctx.counter(k) for k in COUNTERS}
    finally:
        ctx.close()
    assert cnt["shortlist_short"] == 0 and cnt["fused_enabled"] == 1, cnt
    if c["nsh"] == 1:   # (one shell per bin: nothing to order a bin's members by, tile skipping cannot be on)
        assert cnt["tile_seen"] == 0 and cnt["tile_skipped"] == 0 and cnt["tile_unloaded"] == 0, cnt
    want, its_o, ch_o, mv, alld = oracles["fit", name].result()
    assert np.array_equal(mv, np.flatnonzero(initial < 0))
    best, second = _min2(alld)
    want_margin = _margin(best, second)
    sizes = np.bincount(initial[initial >= 0], minlength=B)
    print(f"\n{name}: {len(mv)} movable x {B} bins, {int((sizes < c['m']).sum())} bins start below m members, "
          f"{int((sizes == 0).sum())} empty; oracle: {its_o} sweeps, changes {ch_o.tolist()}, smallest margin "
          f"{want_margin.min():.3e}; counters {cnt}")
    assert want_margin.min() > 4 * QP_TOL   # (the data, not the library: label equality is a fair demand)
    assert its == its_o and np.array_equal(ch, ch_o), (name, its, its_o, ch, ch_o)
    assert np.array_equal(lab, want), (name, np.count_nonzero(lab != want))
    seeds = initial >= 0
    assert np.all(np.isnan(mind[seeds])) and np.all(np.isnan(margin[seeds]))
    assert not np.isnan(mind[mv]).any() and not np.isnan(margin[mv]).any()
    assert np.array_equal(np.isinf(mind[mv]), np.isinf(best))
    fin = np.isfinite(best)
    assert np.all(np.abs(mind[mv] - best)[fin] <= QP_TOL), (name, np.abs(mind[mv] - best)[fin].max())
    assert np.array_equal(np.isinf(margin[mv]), np.isinf(want_margin))
    fin = np.isfinite(want_margin)
    assert np.all(np.abs(margin[mv] - want_margin)[fin] <= 2 * QP_TOL), (name, np.abs(margin[mv] - want_margin)[fin].max())


DEV_NAMES = [n for n in FIT_NAMES if FIT_CASES[n]["dev"]]


@pytest.fixture(scope="module")
def dev_run(tmp_path_factory):
    """One developer-library child (test_gpu_bin_distances.py's) over the cases with B <= 1100: CHB_DEV_ALL_DIST dumps with
    the shortlist stage's checks on."""
    if not os.path.exists(DEV_LIB):
        pytest.fail("developer library not built (__graft_entry__.build() makes it)")
    tmp = tmp_path_factory.mktemp("many_bins")
    cases = []
    for name in DEV_NAMES:
        c = FIT_CASES[name]
        X, initial, perms = fit_data(name)
        npz = str(tmp / f"{name}.npz")
        np.savez(npz, X=X, initial=initial, perms=perms)
        cases.append(dict(name=name, npz=npz, B=c["B"], m=c["m"], its=c["its"], batch=0, metric=None, env={},
                          dump=str(tmp / f"{name}.f64"), out=str(tmp / f"{name}_out.npz")))
    job = dict(root=ROOT, cases=cases, counters=COUNTERS, result=str(tmp / "dev.json"))
    (tmp / "job.json").write_text(json.dumps(job))
    (tmp / "child.py").write_text(CHILD)
    e = dict(os.environ, CHBIN_LIB=DEV_LIB, CHB_SL_BOUNDS="1", CHB_SL_VALIDATE="1")
    p = subprocess.run([sys.executable, str(tmp / "child.py"), str(tmp / "job.json")], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads((tmp / "dev.json").read_text())
    out = {}
    for c in cases:
        N = FIT_CASES[c["name"]]["N"]
        alld = np.fromfile(c["dump"], dtype=np.float64)
        assert alld.size == N * c["B"], (c["name"], alld.size)
        out[c["name"]] = (res[c["name"]], alld.reshape(N, c["B"]), dict(np.load(c["out"])))
        os.remove(c["dump"])
    return out


@pytest.mark.parametrize("name", DEV_NAMES)
def test_dev_all_distances(oracles, dev_run, name):
    """Developer library: every entry of the n_move x B matrix of the last sweep against the oracle."""
    rec, got, outs = dev_run[name]
    want, its_o, ch_o, mv, alld = oracles["fit", name].result()
    assert rec["its"] == its_o and np.array_equal(outs["changed"], ch_o) and np.array_equal(outs["labels"], want)
    assert rec["counters"]["shortlist_short"] == 0 and rec["counters"]["fused_enabled"] == 1, rec["counters"]
    seeds = np.ones(len(got), dtype=bool)
    seeds[mv] = False
    assert np.all(np.isnan(got[seeds])) and not np.any(np.isnan(got[mv]))
    g = got[mv]
    assert np.array_equal(np.isinf(g), np.isinf(alld)), (name, np.argwhere(np.isinf(g) != np.isinf(alld))[:8])
    fin = np.isfinite(alld)
    err = np.abs(g[fin] - alld[fin])
    bad = np.flatnonzero(err > QP_TOL)
    assert bad.size == 0, (name, f"{bad.size} of {err.size} distances off, worst {err.max():.3g}")
    best, second = _min2(g)
    assert np.array_equal(outs["mind"][mv], best) and np.array_equal(outs["margin"][mv], _margin(best, second))
    print(f"\n{name}: {int(fin.sum())} finite + {int((~fin).sum())} +inf distances, worst error {err.max():.3g}; "
          f"counters {rec['counters']}")


def test_tile_skipping_at_16_shells():
    """B = 300 with five coverage columns: 16 shells per bin instead of 32, about 80 members (three 32-row tiles) per bin,
    batches of 2048 so that the fit's verdict on the skipping (taken after three batches) falls.  The fit must equal a
    CHB_TILE_SKIP=0 context, and the oracle replays the last 8 visits of the last sweep.
    On an MI355X the fit sees 2544 wave-tiles in its first batches, skips none of them and turns the skipping off
    (tile_skip_state -1; 2 sweeps, 15000 and 6 changes): whether it stays on is the fit's own decision, so either verdict
    passes."""
    from chbin_amd import _lib, synth
    from oracle import oracle as O
    N, D, S, B, m, its, batch = 24000, 140, 5, 300, 5, 2, 2048
    assert shells_per_bin(B) == 16
    X, initial, _ = synth.make_synthetic(N, D, B, S=S, seed=N + D + B + m, sigma=2e-3, mix=0.2, n_seed=30)
    perms = synth.draw_permutations(initial, its, seed=0)
    a = _lib.Context(0)
    try:
        a.set_samples(X)
        got, its_a, changed = a.fit_cluster(B, initial, perms, m, its, batch=batch)
        state, unloaded = a.counter("tile_skip_state"), a.counter("tile_unloaded")
        skipped, seen = a.counter("tile_skipped"), a.counter("tile_seen")
        assert a.counter("shortlist_short") == 0 and a.counter("fused_enabled") == 1
    finally:
        a.close()
    print(f"\ntile skipping at B = {B}: state {state}, seen {seen}, skipped {skipped}, unloaded {unloaded}; "
          f"{its_a} sweeps, changes {changed.tolist()}")
    assert seen > 0 and state in (1, -1), (state, seen)
    b = _ctx_env({"CHB_TILE_SKIP": "0"})
    try:
        b.set_samples(X)
        want, its_w, changed_w = b.fit_cluster(B, initial, perms, m, its, batch=batch)
        assert b.counter("tile_unloaded") == 0 and b.counter("tile_seen") == 0
        prev = initial
        if its_a > 1:
            prev, _, _ = b.fit_cluster(B, initial, perms[:its_a - 1], m, its_a - 1, batch=batch)
    finally:
        b.close()
    assert its_a == its_w and np.array_equal(changed, changed_w) and np.array_equal(got, want)
    tail = perms[its_a - 1][-8:]
    for k, j in enumerate(tail):
        lab_now = got.copy()
        lab_now[tail[k:]] = prev[tail[k:]]
        lab_j, _ = O.sweep(X, B, lab_now, np.array([j]), m)
        assert lab_j[j] == got[j]


# ---------------------------------------------------------------------------------------------- 5. the limit itself

def test_more_than_8192_bins_is_refused_and_the_context_lives():
    import ctypes as C

    from chbin_amd import _lib, synth
    from oracle import oracle as O
    N, D, B, m, its = 600, 16, 5, 3, 2
    X, initial, _ = synth.make_synthetic(N, D, B, seed=N + D + B + m, sigma=6e-3, mix=0.3)
    perms = synth.draw_permutations(initial, its, seed=0)
    want, its_o, ch_o = O.fit_cluster(X, B, initial, perms, m, its)
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib
        ctx.set_samples(X)

        def usable():
            lab, n, ch = ctx.fit_cluster(B, initial, perms, m, its)
            assert n == its_o and np.array_equal(ch, ch_o) and np.array_equal(lab, want)

        usable()
        out = np.full(N, -5, dtype=np.int64)
        changed = np.zeros(its, dtype=np.int64)
        n = C.c_int(-5)
        rc = lib.chb_fit_cluster(ctx._h, 8193, initial, perms, perms.shape[1], m, its, 0, out, C.byref(n), changed, None)
        assert rc == EUNSUPPORTED and b"8192" in lib.chb_last_error()
        assert np.all(out == -5)
        usable()
        q = np.arange(4, dtype=np.int64)
        idx = np.full((4, 8193, m), -5, dtype=np.int64)
        cnt = np.full((4, 8193), -5, dtype=np.int32)
        rc = lib.chb_topm_per_bin(ctx._h, initial, 8193, m, q, 4, idx, None, cnt)
        assert rc == EUNSUPPORTED and b"8192" in lib.chb_last_error()
        assert np.all(idx == -5) and np.all(cnt == -5)
        usable()
        rc = lib.chb_fit_begin(ctx._h, 8193, initial, m)
        assert rc == EUNSUPPORTED and b"8192" in lib.chb_last_error()
        usable()
        # (and a stepwise fit can still be opened)
        ctx.fit_begin(B, initial, m)
        assert np.array_equal(ctx.fit_labels(), initial)
        ctx.set_samples(X)
        usable()
    finally:
        ctx.close()
