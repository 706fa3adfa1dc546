"""The bindings of the chb_*_wide calls, how the clustering mirrors route num_neighbors to them (stand-in context), and
the oracle's own envelope on the data the GPU tests of test_gpu_wide_m.py compare against (no GPU needed)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import row_reference
import wide_m_cases as W
from chbin_amd import _lib, clustering
from chbin_amd.clustering import algorithm


def test_bound_and_exported():
    lib = _lib.load()
    p, i64, i = C.c_void_p, C.c_int64, C.c_int
    want = {
        # (ctx, labels, groups, B, m, row_idx, Q, bin_out, dist_out, min_dist_out, margin_out)
        "chb_audit_rows_wide": (i, [p, p, p, i64, i, p, i64, p, p, p, p]),
        # (ctx, labels, B, m, Y, Q, D, bin_out, dist_out, min_dist_out, margin_out)
        "chb_recruit_rows_wide": (i, [p, p, i64, i, p, i64, i64, p, p, p, p]),
        # (ctx, labels, groups, B, m, row_idx, bin_idx, P, dist_out, idx_out)
        "chb_audit_pairs_wide": (i, [p, p, p, i64, i, p, p, i64, p, p]),
        # (ctx, labels, B, m, Y, Q, D, row_of, bin_idx, P, dist_out, idx_out)
        "chb_recruit_pairs_wide": (i, [p, p, i64, i, p, i64, i64, p, p, i64, p, p]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == sig
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype is i
    for name in ("audit_rows_wide", "recruit_rows_wide", "audit_pairs_wide", "recruit_pairs_wide"):
        assert callable(getattr(_lib.Context, name))
    # a null context is refused by the library itself, without a device: at an m that forwards and at one that does not
    for m in (5, 17, 64, 65):
        assert lib.chb_audit_rows_wide(None, None, None, 1, m, None, 0, None, None, None, None) == -1
        assert lib.chb_recruit_rows_wide(None, None, 1, m, None, 0, 1, None, None, None, None) == -1
        assert lib.chb_audit_pairs_wide(None, None, None, 1, m, None, None, 0, None, None) == -1
        assert lib.chb_recruit_pairs_wide(None, None, 1, m, None, 0, 1, None, None, 0, None, None) == -1


class StandIn:
    """What the mirror functions use of a Context: every scoring method records (name, m, groups) and answers zeros; the
    wide ones refuse more than 64 neighbours the way the library's refusal reaches a caller."""

    def __init__(self):
        self.calls = []

    def set_samples_cached(self, X):
        self.N = len(X)

    def using_metric(self, metric):
        return contextlib.nullcontext(self)

    def _rows(self, name, m, n, B, groups=None):
        self.calls.append((name, m, groups))
        if name.endswith("_wide") and m > 64:
            raise _lib.ChbError("libchbin_hip error -5: supports at most 64 neighbours")
        return np.zeros(n, dtype=np.int64), np.zeros((n, B)), np.zeros(n), np.zeros(n)

    def _pairs(self, name, m, n, groups=None):
        self.calls.append((name, m, groups))
        if name.endswith("_wide") and m > 64:
            raise _lib.ChbError("libchbin_hip error -5: supports at most 64 neighbours")
        return np.zeros(n)

    def audit_rows(self, labels, B, m, rows=None, want_dist=True):
        return self._rows("audit_rows", m, self.N if rows is None else len(rows), B)

    def audit_rows_grouped(self, labels, groups, B, m, rows=None, want_dist=True):
        return self._rows("audit_rows_grouped", m, self.N if rows is None else len(rows), B, groups)

    def audit_rows_wide(self, labels, B, m, rows=None, want_dist=True, groups=None):
        return self._rows("audit_rows_wide", m, self.N if rows is None else len(rows), B, groups)

    def recruit_rows(self, labels, B, m, Y, want_dist=True):
        return self._rows("recruit_rows", m, len(Y), B)

    def recruit_rows_wide(self, labels, B, m, Y, want_dist=True):
        return self._rows("recruit_rows_wide", m, len(Y), B)

    def audit_pairs(self, labels, B, m, rows, bins):
        return self._pairs("audit_pairs", m, len(rows))

    def audit_pairs_grouped(self, labels, groups, B, m, rows, bins):
        return self._pairs("audit_pairs_grouped", m, len(rows), groups)

    def audit_pairs_wide(self, labels, B, m, rows, bins, groups=None, want_idx=False):
        return self._pairs("audit_pairs_wide", m, len(rows), groups)

    def recruit_pairs(self, labels, B, m, Y, row_of, bins):
        return self._pairs("recruit_pairs", m, len(row_of))

    def recruit_pairs_wide(self, labels, B, m, Y, row_of, bins, want_idx=False):
        return self._pairs("recruit_pairs_wide", m, len(row_of))

    def audit_rows_multi(self, labels, B, ms, rows=None, want_dist=True):
        if max(ms) > 16:
            raise _lib.ChbError("libchbin_hip error -5: chb_audit_rows_multi supports at most 16 neighbours")
        raise AssertionError("not part of these tests")


@pytest.fixture
def standin(monkeypatch):
    s = StandIn()
    monkeypatch.setattr(algorithm, "default_context", lambda: s)
    return s


def test_the_mirrors_split_at_16(standin):
    X, Y = np.zeros((6, 3)), np.ones((4, 3))
    labels = np.array([0, 1, 0, 1, -1, 1], dtype=np.int64)
    groups = np.array([0, 0, 1, 1, -1, 2], dtype=np.int64)

    def last():
        return standin.calls[-1]

    clustering.audit(X, labels, 2, num_neighbors=16)
    assert last() == ("audit_rows", 16, None)
    clustering.audit(X, labels, 2, num_neighbors=16, groups=groups)
    assert last()[:2] == ("audit_rows_grouped", 16) and last()[2] is groups
    clustering.audit(X, labels, 2, num_neighbors=17)
    assert last() == ("audit_rows_wide", 17, None)
    clustering.audit(X, labels, 2, num_neighbors=64, groups=groups)
    assert last()[:2] == ("audit_rows_wide", 64) and last()[2] is groups

    clustering.recruit(X, labels, Y, 2, num_neighbors=16)
    assert last() == ("recruit_rows", 16, None)
    clustering.recruit(X, labels, Y, 2, num_neighbors=17)
    assert last() == ("recruit_rows_wide", 17, None)

    clustering.audit_pairs(X, labels, [0, 1], [1, 0], 2, num_neighbors=16)
    assert last() == ("audit_pairs", 16, None)
    clustering.audit_pairs(X, labels, [0, 1], [1, 0], 2, num_neighbors=16, groups=groups)
    assert last()[:2] == ("audit_pairs_grouped", 16)
    clustering.audit_pairs(X, labels, [0, 1], [1, 0], 2, num_neighbors=17, groups=groups)
    assert last()[:2] == ("audit_pairs_wide", 17) and last()[2] is groups
    clustering.recruit_pairs(X, labels, Y, [0, 1], [1, 0], 2, num_neighbors=16)
    assert last() == ("recruit_pairs", 16, None)
    clustering.recruit_pairs(X, labels, Y, [0, 1], [1, 0], 2, num_neighbors=33)
    assert last() == ("recruit_pairs_wide", 33, None)

    clustering.cohesion(X, labels, 2, num_neighbors=16)
    assert last() == ("audit_pairs", 16, None)
    clustering.cohesion(X, labels, 2, num_neighbors=16, groups=groups)
    assert last()[:2] == ("audit_pairs_grouped", 16)
    clustering.cohesion(X, labels, 2, num_neighbors=17)
    assert last() == ("audit_pairs_wide", 17, None)
    clustering.cohesion(X, labels, 2, num_neighbors=48, groups=groups)
    assert last()[:2] == ("audit_pairs_wide", 48) and last()[2] is groups

    # past 64 the library refuses, and the refusal is what the caller sees
    for call in (lambda: clustering.audit(X, labels, 2, num_neighbors=65),
                 lambda: clustering.recruit(X, labels, Y, 2, num_neighbors=65),
                 lambda: clustering.audit_pairs(X, labels, [0], [0], 2, num_neighbors=65),
                 lambda: clustering.cohesion(X, labels, 2, num_neighbors=65)):
        with pytest.raises(_lib.ChbError, match="at most 64 neighbours"):
            call()
        assert last()[0].endswith("_wide") and last()[1] == 65
    # the list form has no wide counterpart
    with pytest.raises(_lib.ChbError, match="at most 16 neighbours"):
        clustering.neighbor_sweep(X, labels, 2, neighbors=(3, 17))


def _envelope(D, m, twins):
    """The oracle on the shifted problems of every (row, bin) of rows = arange(0, N, 7): feasible weights, a duality gap
    below 1e-10 of the scale, and every row clear."""
    from oracle import oracle as O
    X, lab, _, _ = W.wide(D, twins=twins)
    rows, ref = W.audit_reference(D, m, twins, every_seventh=True)
    assert np.array_equal(rows, np.arange(0, W.N, 7))
    worst_gap, worst_sum, worst_neg = 0.0, 0.0, 0.0
    zero = np.zeros(D)
    for q, r in enumerate(rows):
        for c in range(W.B):
            idx = ref.sets[q][c]
            if len(idx) == 0:
                assert ref.dist[q, c] == np.inf
                continue
            assert len(idx) == min(m, W.SIZES[c] - (lab[r] == c))
            P = np.ascontiguousarray(X[idx] - X[r])
            d, alpha = O.convex_hull_distance(zero, P, return_alpha=True)
            worst_sum = max(worst_sum, abs(alpha.sum() - 1.0))
            worst_neg = max(worst_neg, -alpha.min())
            z = alpha @ P
            nz = np.linalg.norm(z)
            gap = nz - (P @ z).min() / nz if nz > 0.0 else 0.0
            worst_gap = max(worst_gap, gap / ref.scale[q, c])
    _, clear = row_reference.clear_rows(ref)
    print(f"D={D} m={m}: gap/scale <= {worst_gap:.2e}, |sum - 1| <= {worst_sum:.2e}, -min(alpha) <= {worst_neg:.2e}, "
          f"clear {clear.sum()}/{len(clear)}")
    assert worst_sum <= 1e-12 and worst_neg <= 1e-12
    assert worst_gap < 1e-10
    assert clear.all()


@pytest.mark.parametrize("m", [17, 33, 64])
def test_the_reference_stays_inside_its_envelope(m):
    _envelope(72, m, 40)


def test_the_reference_stays_inside_its_envelope_d21():
    _envelope(21, 17, 40)   # (independent sets only: 17 vertices in 21 dimensions)
