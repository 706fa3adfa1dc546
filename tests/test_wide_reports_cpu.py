"""The bindings of chb_audit_rows_nearest_wide, chb_recruit_rows_nearest_wide, chb_bin_report_wide and the two
chb_*_pairs_witness_wide calls, and how clustering.nearest_bins / recruit_nearest_bins / bin_report / witness /
recruit_witness route num_neighbors to them (stand-in context; no GPU needed)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from chbin_amd import _lib, clustering
from chbin_amd.clustering import algorithm

NAMES = ("audit_rows_nearest_wide", "recruit_rows_nearest_wide", "bin_report_wide", "audit_pairs_witness_wide",
         "recruit_pairs_witness_wide")


def test_bound_and_exported():
    lib = _lib.load()
    p, i64, i = C.c_void_p, C.c_int64, C.c_int
    want = {
        # (ctx, labels, groups, B, m, k, row_idx, Q, near_bin, near_dist)
        "chb_audit_rows_nearest_wide": (i, [p, p, p, i64, i, i, p, i64, p, p]),
        # (ctx, labels, B, m, k, Y, Q, D, near_bin, near_dist)
        "chb_recruit_rows_nearest_wide": (i, [p, p, i64, i, i, p, i64, i64, p, p]),
        # (ctx, labels, groups, B, m, row_idx, Q, confusion, unplaced, dcnt, dmin, dsum, n_skipped)
        "chb_bin_report_wide": (i, [p, p, p, i64, i, p, i64, p, p, p, p, p, p]),
        # (ctx, labels, groups, B, m, row_idx, bin_idx, P, dist_out, nbr_idx, nbr_dist, alpha)
        "chb_audit_pairs_witness_wide": (i, [p, p, p, i64, i, p, p, i64, p, p, p, p]),
        # (ctx, labels, B, m, Y, Q, D, row_of, bin_idx, P, dist_out, nbr_idx, nbr_dist, alpha)
        "chb_recruit_pairs_witness_wide": (i, [p, p, i64, i, p, i64, i64, p, p, i64, p, p, p, p]),
    }
    assert set(want) == {"chb_" + n for n in NAMES}
    for name, sig in want.items():
        assert hasattr(lib, name)
        assert _lib.SIGNATURES[name] == sig
        assert getattr(lib, name).argtypes == sig[1] and getattr(lib, name).restype is i
    for name in NAMES:
        assert callable(getattr(_lib.Context, name))
    # a null context is refused by the library itself, without a device: at an m that forwards and at one that does not
    for m in (5, 17, 64, 65):
        assert lib.chb_audit_rows_nearest_wide(None, None, None, 1, m, 1, None, 0, None, None) == -1
        assert lib.chb_recruit_rows_nearest_wide(None, None, 1, m, 1, None, 0, 1, None, None) == -1
        assert lib.chb_bin_report_wide(None, None, None, 1, m, None, 0, None, None, None, None, None, None) == -1
        assert lib.chb_audit_pairs_witness_wide(None, None, None, 1, m, None, None, 0, None, None, None, None) == -1
        assert lib.chb_recruit_pairs_witness_wide(None, None, 1, m, None, 0, 1, None, None, 0, None, None, None, None) == -1


class StandIn:
    """What the mirror functions use of a Context: every method records (name, m, groups) and answers zeros of the
    right shapes; the wide ones refuse more than 64 neighbours the way the library's refusal reaches a caller."""

    def __init__(self):
        self.calls = []

    def set_samples_cached(self, X):
        self.N = len(X)

    def using_metric(self, metric):
        return contextlib.nullcontext(self)

    def _note(self, name, m, groups=None):
        self.calls.append((name, m, groups))
        if name.endswith("_wide") and m > 64:
            raise _lib.ChbError(f"libchbin_hip error -5: chb_{name} supports at most 64 neighbours")

    def _nearest(self, name, m, k, n, groups=None):
        self._note(name, m, groups)
        return np.zeros((n, k), dtype=np.int64), np.zeros((n, k))

    def _report(self, name, m, B, groups=None):
        self._note(name, m, groups)
        z = np.zeros((B, B))
        return z.astype(np.int64), np.zeros(B, dtype=np.int64), z.astype(np.int64), z, z, 0

    def _witness(self, name, m, n, groups=None):
        self._note(name, m, groups)
        return np.zeros(n), np.zeros((n, m), dtype=np.int64), np.zeros((n, m)), np.zeros((n, m))

    def audit_rows_nearest(self, labels, B, m, k, rows=None, groups=None):
        return self._nearest("audit_rows_nearest", m, k, self.N if rows is None else len(rows), groups)

    def audit_rows_nearest_wide(self, labels, B, m, k, rows=None, groups=None):
        return self._nearest("audit_rows_nearest_wide", m, k, self.N if rows is None else len(rows), groups)

    def recruit_rows_nearest(self, labels, B, m, k, Y):
        return self._nearest("recruit_rows_nearest", m, k, len(Y))

    def recruit_rows_nearest_wide(self, labels, B, m, k, Y):
        return self._nearest("recruit_rows_nearest_wide", m, k, len(Y))

    def bin_report(self, labels, B, m, rows=None, groups=None):
        return self._report("bin_report", m, B, groups)

    def bin_report_grouped(self, labels, groups, B, m, rows=None):
        return self._report("bin_report_grouped", m, B, groups)

    def bin_report_wide(self, labels, B, m, rows=None, groups=None):
        return self._report("bin_report_wide", m, B, groups)

    def audit_pairs_witness(self, labels, B, m, rows, bins, groups=None):
        return self._witness("audit_pairs_witness", m, len(rows), groups)

    def audit_pairs_witness_wide(self, labels, B, m, rows, bins, groups=None):
        return self._witness("audit_pairs_witness_wide", m, len(rows), groups)

    def recruit_pairs_witness(self, labels, B, m, Y, row_of, bins):
        return self._witness("recruit_pairs_witness", m, len(row_of))

    def recruit_pairs_witness_wide(self, labels, B, m, Y, row_of, bins):
        return self._witness("recruit_pairs_witness_wide", m, len(row_of))

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
    pr, pb = [0, 1], [1, 0]

    def last():
        return standin.calls[-1]

    # (mirror, its call at m <= 16 without / with groups, its wide call); None: the mirror takes no groups
    audits = (
        (lambda m, g: clustering.nearest_bins(X, labels, 2, k=2, num_neighbors=m, groups=g),
         "audit_rows_nearest", "audit_rows_nearest", "audit_rows_nearest_wide"),
        (lambda m, g: clustering.bin_report(X, labels, 2, num_neighbors=m, groups=g),
         "bin_report", "bin_report_grouped", "bin_report_wide"),
        (lambda m, g: clustering.witness(X, labels, pr, pb, 2, num_neighbors=m, groups=g),
         "audit_pairs_witness", "audit_pairs_witness", "audit_pairs_witness_wide"),
    )
    for call, plain, grouped, wide in audits:
        out = call(16, None)
        assert last() == (plain, 16, None)
        call(16, groups)
        assert last()[:2] == (grouped, 16) and last()[2] is groups
        for m in (17, 64):
            wide_out = call(m, None)
            assert last() == (wide, m, None)
            call(m, groups)
            assert last()[:2] == (wide, m) and last()[2] is groups
            assert type(wide_out) is type(out)   # (the same dataclass, whichever call made it)
        with pytest.raises(_lib.ChbError, match="at most 64 neighbours"):
            call(65, None)
        assert last()[:2] == (wide, 65)
    recruits = (
        (lambda m: clustering.recruit_nearest_bins(X, labels, Y, 2, k=2, num_neighbors=m),
         "recruit_rows_nearest", "recruit_rows_nearest_wide"),
        (lambda m: clustering.recruit_witness(X, labels, Y, pr, pb, 2, num_neighbors=m),
         "recruit_pairs_witness", "recruit_pairs_witness_wide"),
    )
    for call, plain, wide in recruits:
        call(16)
        assert last() == (plain, 16, None)
        for m in (17, 64):
            call(m)
            assert last() == (wide, m, None)
        with pytest.raises(_lib.ChbError, match="at most 64 neighbours"):
            call(65)
        assert last()[:2] == (wide, 65)
    # the shapes follow num_neighbors: m slots per pair at wide m, not 16
    w = clustering.witness(X, labels, pr, pb, 2, num_neighbors=24)
    assert w.neighbors.shape == (2, 24) and w.weights.shape == (2, 24)
    # the list form has no wide counterpart
    with pytest.raises(_lib.ChbError, match="at most 16 neighbours"):
        clustering.neighbor_sweep(X, labels, 2, neighbors=(3, 17))
