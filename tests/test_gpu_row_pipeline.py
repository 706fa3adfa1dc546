"""The chunk pipeline behind chb_audit_rows / chb_recruit_rows / chb_*_rows_multi / chb_bin_report over three and more
chunks, so that a half of the double buffer is used again: chunk k waits for the upload, the kernels and the download of
chunk k - 2.

Every call here is held against the same call on few enough rows for one chunk (or, for the lists, against the single-m
calls): device against device and bit for bit (`same`), so no tolerance is involved.  The positions repeat the 1500
samples / the 70 new rows of test_gpu_neighbor_sweep.sweep_data() cyclically, which makes the expectation of a position an
index into the one-chunk answer."""
import numpy as np
import pytest

from test_gpu_bin_report import check_report, expected
from test_gpu_neighbor_sweep import B, N, check_slices, same, sweep_data

pytestmark = pytest.mark.gpu

CHUNK = 16384


@pytest.fixture(scope="module")
def ctx():
    from chbin_amd import _lib
    c = _lib.Context(0)
    c.set_samples(sweep_data()[0])
    assert c.counter("recruit_chunk") == CHUNK
    yield c
    c.close()


def profiled(ctx, name, call):
    """(call's result, the profile entry `name` of that call alone)"""
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        return out, ctx.profile_get(name)
    finally:
        ctx.profile_enable(False)


def test_audit_three_chunks(ctx):
    _, labels, _ = sweep_data()
    Q, m = 2 * CHUNK + 1, 3
    rows = np.arange(Q, dtype=np.int64) % N
    one = ctx.audit_rows(labels, B, m)
    got, p = profiled(ctx, "audit", lambda: ctx.audit_rows(labels, B, m, rows))
    assert p["launches"] == 3 and p["work"] == Q * B
    for g, w in zip(got, one):
        same(g, w[rows])
    bins, dist, mind, margin = ctx.audit_rows(labels, B, m, rows, want_dist=False)
    assert dist is None
    same(bins, one[0][rows]); same(mind, one[2][rows]); same(margin, one[3][rows])


def test_recruit_three_chunks(ctx):
    _, labels, Y0 = sweep_data()
    Q, m = 2 * CHUNK + 1, 5
    src = np.arange(Q) % len(Y0)
    Y = np.ascontiguousarray(Y0[src])
    one = ctx.recruit_rows(labels, B, m, Y0)
    got, p = profiled(ctx, "recruit", lambda: ctx.recruit_rows(labels, B, m, Y))
    assert p["launches"] == 3
    for g, w in zip(got, one):
        same(g[:len(Y0)], w)       # the first 70 rows
        same(g, g[src])            # every repeat equals its first occurrence


def test_audit_list_of_16(ctx):
    _, labels, _ = sweep_data()
    rng = np.random.default_rng(16)
    ms = tuple(int(m) for m in rng.permutation(16) + 1)
    Q = 4 * 1024 + 71
    rows = rng.integers(0, N, Q).astype(np.int64)
    assert len(np.unique(rows)) < Q
    multi, p = profiled(ctx, "audit_multi", lambda: ctx.audit_rows_multi(labels, B, ms, rows))
    assert ctx.counter("recruit_multi_rows") == 1024
    assert p["launches"] == 5 and p["work"] == Q * B * 16
    check_slices(multi, [ctx.audit_rows(labels, B, m, rows) for m in ms])


def test_recruit_list_of_7(ctx):
    _, labels, Y0 = sweep_data()
    ms = (16, 1, 5, 3, 8, 2, 11)   # chunks of 16384 / 7 rows in whole 64-row tiles: 2304 = upload pieces of 2048 + 256
    Q = 3 * 2304 + 5
    Y = np.ascontiguousarray(Y0[np.arange(Q) % len(Y0)])
    multi, p = profiled(ctx, "recruit_multi", lambda: ctx.recruit_rows_multi(labels, B, ms, Y))
    assert ctx.counter("recruit_multi_rows") == 2304
    assert p["launches"] == 4
    check_slices(multi, [ctx.recruit_rows(labels, B, m, Y) for m in ms])


def test_bin_report_three_chunks(ctx):
    _, labels, _ = sweep_data()
    Q, m = 40000, 2
    rows = np.arange(Q, dtype=np.int64) % N
    bins, dist, _, _ = ctx.audit_rows(labels, B, m, rows)
    got, p = profiled(ctx, "bin_report", lambda: ctx.bin_report(labels, B, m, rows))
    assert Q - got[5] > 2 * CHUNK and p["launches"] >= 3
    check_report("three_chunks", got, expected(labels, B, rows, bins, dist))
    # the guaranteed order (include/chbin_hip.h): a label's rows in blocks of 64, each block in order, the block sums in order
    own = labels[rows]
    want = np.zeros((B, B))
    for a in range(B):
        d = dist[own == a]
        for b in range(B):
            total = 0.0
            for r0 in range(0, len(d), 64):
                s = 0.0
                for v in d[r0:r0 + 64, b]:
                    if np.isfinite(v):
                        s = s + float(v)
                total = total + s
            want[a, b] = total
    assert np.array_equal(got[4].view(np.uint64), want.view(np.uint64))
    again = ctx.bin_report(labels, B, m, rows)
    assert np.array_equal(got[4].view(np.uint64), again[4].view(np.uint64))
    for x, y in zip(got, again):
        assert np.array_equal(x, y)
