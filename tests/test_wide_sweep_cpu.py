"""The bindings of chb_audit_rows_multi_wide / chb_recruit_rows_multi_wide and clustering.neighbor_sweep_wide on a stand-in
context and without a device (no GPU needed)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from chbin_amd import _lib, clustering
from chbin_amd.clustering import algorithm


def test_bound_and_exported():
    import chbin_amd
    lib = _lib.load()
    p, i64, i = C.c_void_p, C.c_int64, C.c_int
    want = {
        # (ctx, labels, groups, B, ms, nm, row_idx, Q, bin_out, dist_out, min_dist_out, margin_out)
        "chb_audit_rows_multi_wide": (i, [p, p, p, i64, p, i, p, i64, p, p, p, p]),
        # (ctx, labels, B, ms, nm, Y, Q, D, bin_out, dist_out, min_dist_out, margin_out)
        "chb_recruit_rows_multi_wide": (i, [p, p, i64, p, i, p, i64, i64, p, p, p, p]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name) and len(sig[1]) == 12
        assert _lib.SIGNATURES[name] == sig
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype is i
    assert callable(_lib.Context.audit_rows_multi_wide) and callable(_lib.Context.recruit_rows_multi_wide)
    assert chbin_amd.neighbor_sweep_wide is clustering.neighbor_sweep_wide and "neighbor_sweep_wide" in chbin_amd.__all__
    assert clustering.neighbor_sweep_wide is algorithm.neighbor_sweep_wide
    assert "neighbor_sweep_wide" in clustering.neighbor_sweep.__doc__
    # a null context is refused by the library itself, without a device: by a list that forwards and by a wide one
    for ms in ((5, 15), (16,), (5, 15, 24, 32, 64), (17,), (65, 3)):
        arr = np.array(ms, dtype=np.intc)
        assert lib.chb_audit_rows_multi_wide(None, None, None, 1, arr.ctypes.data, len(ms), None, 0, None, None, None, None) == -1
        assert lib.chb_recruit_rows_multi_wide(None, None, 1, arr.ctypes.data, len(ms), None, 0, 1, None, None, None, None) == -1
    assert lib.chb_audit_rows_multi_wide(None, None, None, 1, None, 3, None, 0, None, None, None, None) == -1


class StandIn:
    """What neighbor_sweep_wide uses of a Context: the call is recorded and answered with recognisable arrays."""

    def __init__(self):
        self.calls = []

    def set_samples_cached(self, X):
        self.N = len(X)

    def using_metric(self, metric):
        self.metric = metric
        return contextlib.nullcontext(self)

    def audit_rows_multi_wide(self, labels, B, ms, rows=None, want_dist=True, groups=None):
        self.calls.append((labels, B, ms, rows, want_dist, groups))
        nm, Q = len(ms), self.N if rows is None else len(rows)
        bins = (np.arange(nm)[:, None] + np.arange(Q)[None, :]) % B
        mind = np.full((nm, Q), 0.25)
        margin = np.full((nm, Q), 0.5)
        margin[0, 0] = 0.0
        return bins.astype(np.int64), np.full((nm, Q, B), 2.0) if want_dist else None, mind, margin

    def audit_rows_multi(self, *a, **k):
        raise AssertionError("neighbor_sweep_wide has one call: the library forwards")

    audit_rows_multi_grouped = audit_rows_multi


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(algorithm, "default_context", lambda: s)
    return s


def test_the_mirror_passes_everything_through(standin):
    X = np.zeros((6, 3))
    labels = np.array([0, 1, 0, 1, -1, 1], dtype=np.int64)
    groups = np.array([0, 0, 1, 1, -1, 2], dtype=np.int64)
    s = clustering.neighbor_sweep_wide(X, labels, 2)
    got = standin.calls[-1]
    assert np.array_equal(got[0], labels) and got[1] == 2 and np.array_equal(got[2], (5, 15, 24, 32, 64))
    assert got[3] is None and got[4] is False and got[5] is None and standin.metric == "convex"
    assert isinstance(s, clustering.NeighborSweep) and s.distances is None and s.num_clusters == 2
    assert np.array_equal(s.neighbors, (5, 15, 24, 32, 64)) and np.array_equal(s.rows, np.arange(6))
    assert np.array_equal(s.own, labels) and s.bins.shape == s.min_dist.shape == s.margin.shape == (5, 6)
    # the helpers read those arrays: entry j chooses bin (j + q) % 2
    want_bins = (np.arange(5)[:, None] + np.arange(6)[None, :]) % 2
    labelled = labels >= 0
    assert np.array_equal(s.moved, ((want_bins != labels[None, :]) & labelled[None, :]).sum(axis=1))
    assert s.agreement[0, 2] == 1.0 and s.agreement[0, 1] == 0.0
    assert not s.stable().any()
    # rows, groups, metric, an unsorted mixed list and the distances
    rows = np.array([4, 0, 0], dtype=np.int64)
    s = clustering.neighbor_sweep_wide(X, labels, 2, neighbors=(40, 3), metric="affine", rows=rows, return_distances=True,
                                       groups=groups)
    got = standin.calls[-1]
    assert np.array_equal(got[2], (40, 3)) and got[3] is rows and got[4] is True and got[5] is groups
    assert standin.metric == "affine"
    assert np.array_equal(s.rows, rows) and np.array_equal(s.own, labels[rows]) and s.distances.shape == (2, 3, 2)
    assert np.array_equal(s.neighbors, (40, 3))
    # the reference's refusals come first, as in every mirror
    with pytest.raises(NotImplementedError):
        clustering.neighbor_sweep_wide(X, labels, 2, metric="euclid")
    assert len(standin.calls) == 2


def test_no_cpu_fallback():
    """Without a GPU the call fails loudly, as the other mirrors do."""
    if _lib.load().chb_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep_wide(np.zeros((4, 4)), np.zeros(4, dtype=np.int64), 1)
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep_wide(np.zeros((4, 4)), np.zeros(4, dtype=np.int64), 1, neighbors=(2, 40), rows=np.array([0]))
