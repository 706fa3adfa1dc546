"""The bindings of chb_audit_pairs_multi / chb_recruit_pairs_multi and clustering.audit_pairs_sweep / recruit_pairs_sweep /
cohesion_sweep on a stand-in context and without a device (no GPU needed)."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from chbin_amd import _lib, clustering
from chbin_amd.clustering import algorithm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENODEVICE = -2


def test_declared_bound_and_exported():
    import chbin_amd
    lib = _lib.load()
    p, i64, i = C.c_void_p, C.c_int64, C.c_int
    want = {
        # (ctx, labels, groups, B, ms, nm, row_idx, bin_idx, P, dist_out)
        "chb_audit_pairs_multi": (i, [p, p, p, i64, p, i, p, p, i64, p]),
        # (ctx, labels, B, ms, nm, Y, Q, D, row_of, bin_idx, P, dist_out)
        "chb_recruit_pairs_multi": (i, [p, p, i64, p, i, p, i64, i64, p, p, i64, p]),
    }
    with open(os.path.join(ROOT, "include", "chbin_hip.h")) as f:
        header = f.read()
    for name, sig in want.items():
        # declared once in the header, with as many arguments as the binding passes
        decl = re.findall(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M)
        assert len(decl) == 1 and len(re.sub(r"/\*.*?\*/", "", decl[0], flags=re.S).split(",")) == len(sig[1])
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == sig
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype is i
    assert callable(_lib.Context.audit_pairs_multi) and callable(_lib.Context.recruit_pairs_multi)
    for name in ("audit_pairs_sweep", "recruit_pairs_sweep", "cohesion_sweep"):
        assert getattr(chbin_amd, name) is getattr(clustering, name) is getattr(algorithm, name) and name in chbin_amd.__all__
    assert "audit_pairs_sweep" in clustering.NearestBins.pairs.__doc__
    # the profile names are documented where chb_profile_get is
    for name in ("audit_pairs_multi", "recruit_pairs_multi", "audit_pairs_multi_wide_select", "audit_pairs_multi_wide_solve"):
        assert '"' + name + '"' in header
    # a null context is refused by the library itself, without a device: narrow, wide and malformed lists alike
    for ms in ((1, 3, 5, 10, 15), (16,), (5, 15, 24, 32, 64), (17,), (65, 3), (0,)):
        arr = np.array(ms, dtype=np.intc)
        assert lib.chb_audit_pairs_multi(None, None, None, 1, arr.ctypes.data, len(ms), None, None, 0, None) == -1
        assert lib.chb_recruit_pairs_multi(None, None, 1, arr.ctypes.data, len(ms), None, 0, 1, None, None, 0, None) == -1
    assert lib.chb_audit_pairs_multi(None, None, None, 1, None, 3, None, None, 0, None) == -1


class StandIn:
    """What the three mirrors use of a Context: the calls are recorded and answered with 100000 * m + 1000 * row + bin."""

    def __init__(self):
        self.calls = []
        self.metrics = []

    def set_samples_cached(self, X):
        self.N = len(X)

    def using_metric(self, metric):
        self.metrics.append(metric)
        return contextlib.nullcontext(self)

    @staticmethod
    def answer(ms, rows, bins):
        return 100000.0 * np.asarray(ms)[:, None] + 1000.0 * np.asarray(rows)[None, :] + np.asarray(bins)[None, :]

    def audit_pairs_multi(self, labels, B, ms, rows, bins, groups=None):
        self.calls.append(("audit", np.array(labels), B, np.array(ms), np.array(rows), np.array(bins), groups))
        return self.answer(ms, rows, bins)

    def recruit_pairs_multi(self, labels, B, ms, Y, row_of, bins):
        self.calls.append(("recruit", np.array(labels), B, np.array(ms), np.array(Y), np.array(row_of), np.array(bins)))
        return self.answer(ms, row_of, bins)

    def audit_pairs(self, *a, **k):
        raise AssertionError("a sweep is one list call, not a call per entry")

    audit_pairs_wide = audit_pairs_grouped = recruit_pairs = recruit_pairs_wide = audit_pairs


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(algorithm, "default_context", lambda: s)
    return s


def test_pair_sweeps_pass_everything_through(standin):
    X, Y = np.zeros((5, 3)), np.ones((4, 3))
    labels = np.array([0, 1, 0, 1, -1], dtype=np.int64)
    groups = np.array([0, 0, 1, 1, -1], dtype=np.int64)
    got = clustering.audit_pairs_sweep(X, labels, [4, 0, 4], [1, 1, 0], 2)
    kind, lab, B, ms, rows, bins, grp = standin.calls[-1]
    assert kind == "audit" and B == 2 and np.array_equal(lab, labels) and grp is None
    assert np.array_equal(ms, (1, 3, 5, 10, 15)) and np.array_equal(rows, [4, 0, 4]) and np.array_equal(bins, [1, 1, 0])
    assert got.shape == (5, 3) and np.array_equal(got, StandIn.answer((1, 3, 5, 10, 15), [4, 0, 4], [1, 1, 0]))
    # an unsorted list on both sides of 16, groups and the metric
    got = clustering.audit_pairs_sweep(X, labels, [2], [0], 2, neighbors=(40, 3, 64), metric="affine", groups=groups)
    assert np.array_equal(standin.calls[-1][3], (40, 3, 64)) and standin.calls[-1][6] is groups
    assert np.array_equal(got[:, 0], [4002000.0, 302000.0, 6402000.0])
    got = clustering.recruit_pairs_sweep(X, labels, Y, [3, 3], [0, 1], 2, neighbors=(24, 2), qp_solver="cvxopt")
    kind, lab, B, ms, Yg, row_of, bins = standin.calls[-1]
    assert kind == "recruit" and B == 2 and np.array_equal(ms, (24, 2)) and np.array_equal(Yg, Y) and Yg.dtype == np.float64
    assert np.array_equal(row_of, [3, 3]) and np.array_equal(bins, [0, 1])
    assert np.array_equal(got, StandIn.answer((24, 2), [3, 3], [0, 1]))
    assert np.array_equal(clustering.recruit_pairs_sweep(X, labels, Y, [0], [0], 2).shape, (5, 1))   # (the default list)
    assert standin.metrics == ["convex", "affine", "convex", "convex"]
    # the reference's refusals come first, as in every mirror
    n = len(standin.calls)
    for fn, args in ((clustering.audit_pairs_sweep, (X, labels, [0], [0], 2)),
                     (clustering.recruit_pairs_sweep, (X, labels, Y, [0], [0], 2)),
                     (clustering.cohesion_sweep, (X, labels, 2))):
        with pytest.raises(NotImplementedError, match="Unknown solver"):
            fn(*args, qp_solver="gurobi")
        with pytest.raises(NotImplementedError, match="Metric"):
            fn(*args, metric="euclid")
    assert len(standin.calls) == n


def test_cohesion_sweep_builds_the_own_bin_list(standin):
    X = np.zeros((8, 3))
    labels = np.array([2, 0, -1, 1, 3, 99, 0, -7], dtype=np.int64)   # 3 = num_clusters: outside
    groups = np.arange(8, dtype=np.int64)
    got = clustering.cohesion_sweep(X, labels, 3, metric="affine")
    (kind, lab, B, ms, rows, bins, grp), = standin.calls
    assert kind == "audit" and B == 3 and np.array_equal(lab, labels) and grp is None and standin.metrics == ["affine"]
    assert np.array_equal(ms, (1, 3, 5, 10, 15))
    assert np.array_equal(rows, [0, 1, 3, 6]) and np.array_equal(bins, [2, 0, 1, 0])   # order kept, the others left out
    assert rows.dtype == np.int64 and bins.dtype == np.int64
    assert got.shape == (5, 8)
    unscored = [False, False, True, False, True, True, False, True]
    assert np.array_equal(np.isnan(got), np.tile(unscored, (5, 1)))
    assert np.array_equal(got[:, [0, 1, 3, 6]], StandIn.answer(ms, [0, 1, 3, 6], [2, 0, 1, 0]))
    # chosen rows with a repeat, an unsorted wide list, groups
    chosen = np.array([6, 2, 0, 6, 4, 3])
    got = clustering.cohesion_sweep(X, labels, 3, neighbors=(33, 2), rows=chosen, groups=groups)
    _, _, _, ms, rows, bins, grp = standin.calls[-1]
    assert np.array_equal(ms, (33, 2)) and grp is groups
    assert np.array_equal(rows, [6, 0, 6, 3]) and np.array_equal(bins, [0, 2, 0, 1])
    assert np.array_equal(np.isnan(got), np.tile([False, True, False, False, True, False], (2, 1)))
    assert np.array_equal(got[:, [0, 2, 3, 5]], StandIn.answer((33, 2), [6, 0, 6, 3], [0, 2, 0, 1]))
    # no row with a label in range: the list is empty and everything is NaN
    got = clustering.cohesion_sweep(X, np.full(8, -1, dtype=np.int64), 3, neighbors=(4, 40, 7))
    assert len(standin.calls[-1][4]) == 0 and np.isnan(got).all() and got.shape == (3, 8)


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_malformed_lists_are_refused_before_the_library():
    ctx = _lib.Context.__new__(_lib.Context)   # (no device: nothing of the library may be reached)
    ctx._lib, ctx._h, ctx.N, ctx.D = NoLibrary(), C.c_void_p(), 6, 3
    labels = np.zeros(6, dtype=np.int64)
    Y = np.zeros((4, 3))
    with pytest.raises(ValueError, match="one entry per pair"):
        ctx.audit_pairs_multi(labels, 2, (5, 20), [0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="one entry per pair"):
        ctx.recruit_pairs_multi(labels, 2, (5, 20), Y, [0, 1], [0, 1, 1])
    with pytest.raises(ValueError, match="1-D list of neighbour counts"):
        ctx.audit_pairs_multi(labels, 2, [[5, 20]], [0, 1], [0, 1])
    with pytest.raises(ValueError, match="one entry per resident sample"):
        ctx.audit_pairs_multi(labels, 2, (5, 20), [0, 1], [0, 1], groups=np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="2-D"):
        ctx.recruit_pairs_multi(labels, 2, (5, 20), Y[0], [0, 1], [0, 1])
    # well-formed lists reach the library
    with pytest.raises(AssertionError, match="chb_audit_pairs_multi"):
        ctx.audit_pairs_multi(labels, 2, (5, 20), [0, 1], [0, 1])
    with pytest.raises(AssertionError, match="chb_recruit_pairs_multi"):
        ctx.recruit_pairs_multi(labels, 2, (5, 20), Y, [0, 1], [0, 1])


def test_no_cpu_fallback():
    """Without a GPU the calls fail loudly with CHB_ENODEVICE, as the other mirrors do."""
    lib = _lib.load()
    if lib.chb_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    assert lib.chb_create(0, C.byref(h)) == ENODEVICE
    X, lab = np.zeros((4, 4)), np.zeros(4, dtype=np.int64)
    for call in (lambda: clustering.cohesion_sweep(X, lab, 1),
                 lambda: clustering.cohesion_sweep(X, lab, 1, neighbors=(2, 40)),
                 lambda: clustering.audit_pairs_sweep(X, lab, [0, 1], [0, 0], 1),
                 lambda: clustering.recruit_pairs_sweep(X, lab, X, [0, 1], [0, 0], 1, neighbors=(64, 1))):
        with pytest.raises(_lib.ChbError, match="no HIP device"):   # (what Context makes of the library's CHB_ENODEVICE)
            call()
