"""clustering.Witness on hand-made arrays against direct numpy, and the argument errors of witness / recruit_witness that
are raised before any context is touched.  No GPU."""
import numpy as np
import pytest

from chbin_amd import clustering
from chbin_amd.clustering import Witness

INF = np.inf


def hand_made():
    """Five samples in four columns and four pairs: a full record, one padded to two vertices, an empty bin, and an affine
    record with a negative weight and a vertex of weight zero."""
    samples = np.array([[0.0, 0.0, 1.0, 2.0],
                        [1.0, 0.0, 0.0, 2.0],
                        [0.0, 2.0, 0.0, 1.0],
                        [4.0, 4.0, 4.0, 4.0],
                        [1.0, 1.0, 1.0, 1.0]])
    neighbors = np.array([[0, 1, 2], [4, 3, -1], [-1, -1, -1], [2, 0, 1]])
    neighbor_dist = np.array([[0.5, 0.6, 0.7], [0.1, 5.0, INF], [INF, INF, INF], [1.0, 2.0, 3.0]])
    weights = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.5, -0.5, 0.0]])
    points = np.array([[0.5, 0.5, 0.5, 1.5], [1.0, 1.0, 1.0, 3.0], [9.0, 9.0, 9.0, 9.0], [0.0, 3.0, 0.0, 0.0]])
    nearest = np.array([0.5 * samples[0] + 0.25 * samples[1] + 0.25 * samples[2],
                        samples[4],
                        np.zeros(4),
                        1.5 * samples[2] - 0.5 * samples[0]])
    dist = np.linalg.norm(points - nearest, axis=1)
    dist[2] = INF
    return samples, points, nearest, Witness(dist, neighbors, neighbor_dist, weights)


def test_count_and_support():
    _, _, _, w = hand_made()
    assert np.array_equal(w.count, [3, 2, 0, 3])
    assert w.support.dtype == bool
    assert np.array_equal(w.support, [[True, True, True], [True, False, False], [False, False, False], [True, True, False]])


def test_nearest_point_skips_padding():
    samples, _, nearest, w = hand_made()
    got = w.nearest_point(samples)
    assert got.shape == (4, 4)
    assert np.allclose(got, nearest, rtol=0, atol=1e-15)
    assert np.all(got[2] == 0.0)
    # padding is skipped whatever its slots hold, also with samples that would turn 0 * x into NaN
    bad = samples.copy()
    bad[0] = INF
    w2 = Witness(w.dist[1:3], w.neighbors[1:3], w.neighbor_dist[1:3], np.array([[1.0, 0.0, 7.0], [3.0, 3.0, 3.0]]))
    got = w2.nearest_point(bad)
    assert np.array_equal(got, [bad[4], np.zeros(4)])


def test_residual_by_block():
    samples, points, nearest, w = hand_made()
    blocks = [(0, 1), (1, 3), (3, 4)]
    got = w.residual_by_block(samples, points, blocks)
    assert got.shape == (4, 3)
    r2 = (points - nearest) ** 2
    want = np.stack([r2[:, 0], r2[:, 1] + r2[:, 2], r2[:, 3]], axis=1)
    keep = [0, 1, 3]
    assert np.allclose(got[keep], want[keep], rtol=0, atol=1e-15)
    assert np.isnan(got[2]).all()                                  # the empty bin's pair has no nearest point
    assert np.allclose(got[keep].sum(axis=1), w.dist[keep] ** 2, rtol=1e-14, atol=0)   # a partition sums to dist**2
    # one block, overlapping blocks, no block
    assert np.allclose(w.residual_by_block(samples, points, [(0, 4)])[keep, 0], w.dist[keep] ** 2, rtol=1e-14, atol=0)
    two = w.residual_by_block(samples, points, [(0, 3), (2, 4)])
    assert np.allclose(two[keep], np.stack([r2[:, :3].sum(axis=1), r2[:, 2:].sum(axis=1)], axis=1)[keep], rtol=0, atol=1e-15)
    assert w.residual_by_block(samples, points, []).shape == (4, 0)


def test_empty_witness():
    w = Witness(np.zeros(0), np.zeros((0, 5), dtype=np.int64), np.zeros((0, 5)), np.zeros((0, 5)))
    assert w.count.shape == (0,) and w.support.shape == (0, 5)
    assert w.nearest_point(np.ones((3, 2))).shape == (0, 2)
    assert w.residual_by_block(np.ones((3, 2)), np.zeros((0, 2)), [(0, 1), (1, 2)]).shape == (0, 2)


def test_argument_errors_come_before_any_context(monkeypatch):
    from chbin_amd.clustering import algorithm

    def no_context(*a, **k):
        raise AssertionError("the context was touched before the arguments were checked")
    monkeypatch.setattr(algorithm, "default_context", no_context)
    X, labels = np.zeros((4, 4)), np.zeros(4, dtype=np.int64)
    with pytest.raises(NotImplementedError, match="Metric manhattan"):
        clustering.witness(X, labels, [0], [0], 1, metric="manhattan")
    with pytest.raises(NotImplementedError, match="Metric manhattan"):
        clustering.recruit_witness(X, labels, X, [0], [0], 1, metric="manhattan")
    with pytest.raises(NotImplementedError):
        clustering.witness(X, labels, [0], [0], 1, qp_solver="nosuch")
    with pytest.raises(NotImplementedError):
        clustering.recruit_witness(X, labels, X, [0], [0], 1, qp_solver="nosuch")
    # (valid arguments do reach the context)
    with pytest.raises(AssertionError, match="context was touched"):
        clustering.witness(X, labels, [0], [0], 1, metric="affine", qp_solver="cvxopt")
