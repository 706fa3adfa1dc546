"""The bindings of chb_audit_pairs / chb_recruit_pairs, the pair lists clustering.cohesion builds and the length checks of
Context.audit_pairs / recruit_pairs, with a stand-in context (no GPU needed)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from chbin_amd import _lib, clustering
from chbin_amd.clustering import algorithm


class StandIn:
    """What the mirror functions use of a Context; audit_pairs answers 1000 * row + bin and records its arguments."""

    def __init__(self):
        self.calls = []
        self.metrics = []

    def set_samples_cached(self, X):
        self.N = len(X)

    def using_metric(self, metric):
        self.metrics.append(metric)
        return contextlib.nullcontext(self)

    def audit_pairs(self, labels, B, m, rows, bins):
        self.calls.append(("audit", np.array(labels), B, m, np.array(rows), np.array(bins)))
        return 1000.0 * np.asarray(rows) + np.asarray(bins)

    def recruit_pairs(self, labels, B, m, Y, row_of, bins):
        self.calls.append(("recruit", np.array(labels), B, m, np.array(Y), np.array(row_of), np.array(bins)))
        return 1000.0 * np.asarray(row_of) + np.asarray(bins)


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(algorithm, "default_context", lambda: s)
    return s


def test_bound_and_exported():
    import chbin_amd
    lib = _lib.load()
    for name in ("chb_audit_pairs", "chb_recruit_pairs"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    p, i64, i = C.c_void_p, C.c_int64, C.c_int
    # (ctx, labels, B, m, row_idx, bin_idx, P, dist_out)
    assert _lib.SIGNATURES["chb_audit_pairs"] == (i, [p, p, i64, i, p, p, i64, p])
    # (ctx, labels, B, m, Y, Q, D, row_of, bin_idx, P, dist_out)
    assert _lib.SIGNATURES["chb_recruit_pairs"] == (i, [p, p, i64, i, p, i64, i64, p, p, i64, p])
    assert lib.chb_audit_pairs.argtypes == _lib.SIGNATURES["chb_audit_pairs"][1]
    assert lib.chb_recruit_pairs.argtypes == _lib.SIGNATURES["chb_recruit_pairs"][1]
    for name in ("audit_pairs", "recruit_pairs", "cohesion"):
        assert getattr(chbin_amd, name) is getattr(clustering, name) and name in chbin_amd.__all__
    assert callable(_lib.Context.audit_pairs) and callable(_lib.Context.recruit_pairs)
    # a null context is refused by the library itself, without a device
    assert lib.chb_audit_pairs(None, None, 1, 1, None, None, 0, None) == -1
    assert lib.chb_recruit_pairs(None, None, 1, 1, None, 0, 1, None, None, 0, None) == -1


def test_cohesion_builds_the_own_bin_list(standin):
    X = np.zeros((8, 3))
    labels = np.array([2, 0, -1, 1, 3, 99, 0, -7], dtype=np.int64)   # 3 = num_clusters: outside
    got = clustering.cohesion(X, labels, 3, num_neighbors=4, metric="affine")
    (kind, lab, B, m, rows, bins), = standin.calls
    assert kind == "audit" and B == 3 and m == 4 and np.array_equal(lab, labels)
    assert np.array_equal(rows, [0, 1, 3, 6]) and np.array_equal(bins, [2, 0, 1, 0])   # order kept, the others left out
    assert rows.dtype == np.int64 and bins.dtype == np.int64
    assert standin.metrics == ["affine"]
    assert got.shape == (8,)
    assert np.array_equal(np.isnan(got), [False, False, True, False, True, True, False, True])
    assert np.array_equal(got[[0, 1, 3, 6]], [2.0, 1000.0, 3001.0, 6000.0])


def test_cohesion_of_chosen_rows(standin):
    X = np.zeros((8, 3))
    labels = np.array([2, 0, -1, 1, 3, 99, 0, -7], dtype=np.int64)
    chosen = np.array([6, 2, 0, 6, 4, 3])   # a repeat, and rows without a label in [0, 3) in between
    got = clustering.cohesion(X, labels, 3, rows=chosen)
    (_, _, B, m, rows, bins), = standin.calls
    assert B == 3 and m == 15
    assert np.array_equal(rows, [6, 0, 6, 3]) and np.array_equal(bins, [0, 2, 0, 1])
    assert np.array_equal(np.isnan(got), [False, True, False, False, True, False])
    assert np.array_equal(got[[0, 2, 3, 5]], [6000.0, 2.0, 6000.0, 3001.0])
    # no row with a label in range: the list is empty and everything is NaN
    standin.calls.clear()
    got = clustering.cohesion(X, np.full(8, -1, dtype=np.int64), 3)
    assert len(standin.calls[0][4]) == 0 and np.isnan(got).all() and got.shape == (8,)


def test_mirrors_pass_the_lists_through(standin):
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    labels = np.array([0, 1, 0, 1, -1], dtype=np.int64)
    got = clustering.audit_pairs(X, labels, [4, 0, 4], [1, 1, 0], 2, num_neighbors=3)
    assert np.array_equal(got, [4001.0, 1.0, 4000.0])
    got = clustering.recruit_pairs(X, labels, Y, [3, 3], [0, 1], 2, metric="affine", qp_solver="cvxopt")
    assert np.array_equal(got, [3000.0, 3001.0])
    assert standin.calls[1][0] == "recruit" and np.array_equal(standin.calls[1][4], Y) and standin.calls[1][3] == 15
    assert standin.metrics == ["convex", "affine"]
    for fn, args in ((clustering.audit_pairs, (X, labels, [0], [0], 2)),
                     (clustering.recruit_pairs, (X, labels, Y, [0], [0], 2)),
                     (clustering.cohesion, (X, labels, 2))):
        with pytest.raises(NotImplementedError, match="Unknown solver"):
            fn(*args, qp_solver="gurobi")
        with pytest.raises(NotImplementedError, match="Metric"):
            fn(*args, metric="euclid")
    assert len(standin.calls) == 2


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_mismatched_lengths_are_refused_before_the_library():
    ctx = _lib.Context.__new__(_lib.Context)   # (no device: nothing of the library may be reached)
    ctx._lib, ctx._h, ctx.N, ctx.D = NoLibrary(), C.c_void_p(), 6, 3
    labels = np.zeros(6, dtype=np.int64)
    Y = np.zeros((4, 3))
    with pytest.raises(ValueError, match="one entry per pair"):
        ctx.audit_pairs(labels, 2, 5, [0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="one entry per pair"):
        ctx.recruit_pairs(labels, 2, 5, Y, [0, 1], [0, 1, 1])
    with pytest.raises(ValueError, match="1-D"):
        ctx.audit_pairs(labels, 2, 5, [[0, 1]], [[0, 1]])
    with pytest.raises(ValueError, match="one entry per resident sample"):
        ctx.audit_pairs(labels[:5], 2, 5, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="2-D"):
        ctx.recruit_pairs(labels, 2, 5, Y[0], [0, 1], [0, 1])
    # well-formed lists reach the library
    with pytest.raises(AssertionError, match="chb_audit_pairs"):
        ctx.audit_pairs(labels, 2, 5, [0, 1], [0, 1])
    with pytest.raises(AssertionError, match="chb_recruit_pairs"):
        ctx.recruit_pairs(labels, 2, 5, Y, [0, 1], [0, 1])

