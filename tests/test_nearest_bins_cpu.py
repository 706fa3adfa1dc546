"""clustering.NearestBins on hand-made arrays, rank_dense -- the numpy definition of chb_*_rows_nearest that the GPU tests
rank the dense calls' tables with -- on a hand-written case, and the refusals that need no GPU."""
import numpy as np
import pytest

from chbin_amd import _lib, clustering
from chbin_amd.clustering import NearestBins

EINVAL = -1
INF = np.inf


def rank_dense(dist, k):
    """(bins [n, k] int64, dist [n, k]) of a dense [n, B] table by include/chbin_hip.h's definition: per row the FINITE
    entries in (distance, bin) ascending order, the first k of them, then bin -1 / +inf.  The distances are moved, never
    recomputed: they keep their bits."""
    dist = np.asarray(dist, dtype=np.float64)
    n = dist.shape[0]
    bins, out = np.full((n, k), -1, dtype=np.int64), np.full((n, k), INF)
    for q in range(n):
        c = np.flatnonzero(np.isfinite(dist[q]))
        c = c[np.lexsort((c, dist[q, c]))][:k]   # (the last key is the primary one)
        bins[q, :len(c)] = c
        out[q, :len(c)] = dist[q, c]
    return bins, out


def test_rank_dense_on_a_hand_written_case():
    d = np.array([[0.5, INF, 0.25, 0.5, 0.25, INF, 0.125],    # two exact ties: (2, 4) and (0, 3)
                  [INF, INF, INF, 3.0, INF, INF, INF],        # one finite entry
                  [INF] * 7,                                  # none
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],        # all tied
                  [7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]])
    bins, dist = rank_dense(d, 4)
    assert bins.dtype == np.int64 and dist.dtype == np.float64
    assert bins.tolist() == [[6, 2, 4, 0], [3, -1, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 3], [6, 5, 4, 3]]
    assert dist.tolist() == [[0.125, 0.25, 0.25, 0.5], [3.0, INF, INF, INF], [INF] * 4, [0.0] * 4, [1.0, 2.0, 3.0, 4.0]]
    # k = 1 is the strict-'>' scan; k > B pads
    assert rank_dense(d, 1)[0][:, 0].tolist() == [6, 3, -1, 0, 6]
    bins, dist = rank_dense(d, 9)
    assert bins.shape == (5, 9) and bins[0].tolist() == [6, 2, 4, 0, 3, -1, -1, -1, -1]
    assert np.all(bins[:, 7:] == -1) and np.all(dist[:, 7:] == INF)
    # the bits travel: a negative zero stays one, and ties with +0.0 go by bin
    z = np.array([[0.0, -0.0, 1.0]])
    bins, dist = rank_dense(z, 2)
    assert bins.tolist() == [[0, 1]] and not np.signbit(dist[0, 0]) and np.signbit(dist[0, 1])


def hand_made():
    bins = np.array([[6, 2, 4], [3, -1, -1], [-1, -1, -1], [0, 1, 2], [5, 1, -1]], dtype=np.int64)
    dist = np.array([[0.125, 0.25, 0.25], [3.0, INF, INF], [INF, INF, INF], [0.0, 0.0, 0.0], [1.0, 1.5, INF]])
    return NearestBins(bins, dist)


def test_count_and_margin_with_padding():
    nb = hand_made()
    assert nb.count.tolist() == [3, 1, 0, 3, 2]
    margin = nb.margin
    assert margin.tolist() == [0.125, INF, INF, 0.0, 0.5]   # (never inf - inf)
    assert not np.isnan(margin).any()


def test_margin_needs_a_runner_up():
    nb = hand_made()
    one = NearestBins(nb.bins[:, :1], nb.dist[:, :1])
    assert one.count.tolist() == [1, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        one.margin
    with pytest.raises(ValueError):
        one.ambiguous(0.1)


def test_ambiguous_and_ties():
    nb = hand_made()
    assert nb.ambiguous(0.0).tolist() == [False, False, False, True, False]      # only the exact tie
    assert nb.ambiguous(0.125).tolist() == [True, False, False, True, False]
    assert nb.ambiguous(1.0).tolist() == [True, False, False, True, True]        # a row without a runner-up never is
    # relative: margin <= tol * nearest distance; 0.125 <= 1.0 * 0.125, 0.5 <= 0.5 * 1.0, 0 <= 0
    assert nb.ambiguous(1.0, relative=True).tolist() == [True, False, False, True, True]
    assert nb.ambiguous(0.4, relative=True).tolist() == [False, False, False, True, False]


def test_pairs():
    nb = hand_made()
    pos, bins = nb.pairs()
    assert pos.dtype == np.int64 and bins.dtype == np.int64
    assert pos.tolist() == [0, 0, 1, 3, 3, 4, 4] and bins.tolist() == [6, 2, 3, 0, 1, 5, 1]   # real entries only, row by row
    pos, bins = nb.pairs(ranks=(1, 2))
    assert pos.tolist() == [0, 0, 3, 3, 4] and bins.tolist() == [2, 4, 1, 2, 1]
    pos, bins = nb.pairs(ranks=(2,), mask=np.array([True, True, True, False, True]))
    assert pos.tolist() == [0] and bins.tolist() == [4]
    pos, bins = nb.pairs(mask=nb.ambiguous(0.2))
    assert pos.tolist() == [0, 0, 3, 3] and bins.tolist() == [6, 2, 0, 1]
    pos, bins = nb.pairs(mask=np.zeros(5, dtype=bool))
    assert pos.shape == (0,) and bins.shape == (0,)
    empty = NearestBins(np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3)))
    assert empty.count.shape == (0,) and empty.margin.shape == (0,) and empty.pairs()[0].shape == (0,)


def test_null_context_is_refused():
    lib = _lib.load()
    labels = np.zeros(4, dtype=np.int64)
    rows = np.arange(4, dtype=np.int64)
    Y = np.zeros((4, 3))
    nb, nd = np.full(12, -5, dtype=np.int64), np.full(12, -5.0)
    assert lib.chb_audit_rows_nearest(None, labels.ctypes.data, None, 2, 5, 3, rows.ctypes.data, 4, nb.ctypes.data,
                                      nd.ctypes.data) == EINVAL
    assert b"null context" in lib.chb_last_error()
    assert lib.chb_recruit_rows_nearest(None, labels.ctypes.data, 2, 5, 3, Y.ctypes.data, 4, 3, nb.ctypes.data,
                                        nd.ctypes.data) == EINVAL
    assert b"null context" in lib.chb_last_error()
    assert np.all(nb == -5) and np.all(nd == -5.0)


def test_mirror_argument_errors_come_before_the_gpu():
    X = np.zeros((4, 3))
    labels = np.zeros(4, dtype=np.int64)
    with pytest.raises(NotImplementedError):
        clustering.nearest_bins(X, labels, 1, metric="manhattan")
    with pytest.raises(NotImplementedError):
        clustering.recruit_nearest_bins(X, labels, X, 1, metric="manhattan")
    with pytest.raises(Exception) as e:
        clustering.nearest_bins(X, labels, 1, qp_solver="nosuch")
    assert not isinstance(e.value, _lib.ChbError)
    with pytest.raises(Exception) as e:
        clustering.recruit_nearest_bins(X, labels, X, 1, qp_solver="nosuch")
    assert not isinstance(e.value, _lib.ChbError)
