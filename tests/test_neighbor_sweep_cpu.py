"""clustering.NeighborSweep's pure-numpy helpers on hand-made arrays, the bindings of chb_audit_rows_multi /
chb_recruit_rows_multi, and neighbor_sweep without a device (no GPU needed)."""
import numpy as np
import pytest

from chbin_amd import _lib, clustering

INF = np.inf


def make_sweep():
    """3 entries of `neighbors`, 8 scored rows, 3 bins.  Rows 0 .. 4 carry a label in [0, 3); row 5 is unassigned (-1), row 6
    carries 99, row 7 carries 3 (= num_clusters: outside)."""
    own = np.array([0, 1, 2, 0, 1, -1, 99, 3], dtype=np.int64)
    bins = np.array([[0, 1, 2, 1, -1, -1, 0, 2],
                     [0, 1, 2, 0, -1, 0, 0, 2],
                     [0, 2, 2, 0, 1, -1, 1, 2]], dtype=np.int64)
    margin = np.array([[0.5, 0.25, INF, 0.125, INF, INF, 0.5, 0.5],
                       [0.25, 0.0, INF, 0.5, INF, 0.5, 0.5, 0.5],
                       [0.75, 0.5, INF, 0.5, 0.5, INF, 0.5, 0.5]])
    mind = np.where(bins >= 0, 0.125, INF)
    rows = np.arange(10, 18, dtype=np.int64)
    return clustering.NeighborSweep(np.array([3, 5, 15]), rows, own, bins, mind, margin, 3)


def test_moved_counts_labelled_rows_only():
    s = make_sweep()
    # m = 3: rows 3 (0 -> 1) and 4 (1 -> none); m = 5: row 4; m = 15: row 1 (1 -> 2).  Rows 5, 6 and 7 have no label in
    # [0, 3) and never count, whatever their bin (row 5's own -1 equals its bin -1 at two entries, differs at one)
    moved = s.moved
    assert moved.shape == (3,) and np.array_equal(moved, [2, 1, 1])
    # every labelled row moved
    t = make_sweep()
    t.bins[0, :5] = [1, 2, 0, -1, -1]
    assert t.moved[0] == 5


def test_agreement_matrix():
    s = make_sweep()
    a = s.agreement
    assert a.shape == (3, 3) and np.array_equal(a, a.T) and np.array_equal(np.diag(a), [1.0, 1.0, 1.0])
    # m = 3 against m = 5: rows 3 and 5 differ; both choosing none (row 4) is the same choice
    assert a[0, 1] == 6 / 8
    # m = 3 against m = 15: rows 1, 3, 4, 6 differ
    assert a[0, 2] == 4 / 8
    # m = 5 against m = 15: rows 1, 4, 5, 6 differ
    assert a[1, 2] == 4 / 8
    empty = clustering.NeighborSweep(np.array([1, 2]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64),
                                     np.zeros((2, 0), dtype=np.int64), np.zeros((2, 0)), np.zeros((2, 0)), 3)
    assert empty.agreement.shape == (2, 2) and np.isnan(empty.agreement).all()
    assert np.array_equal(empty.moved, [0, 0]) and empty.stable().shape == (0,)


def test_stable_rows():
    s = make_sweep()
    # row 0: own bin at every entry, margins 0.5 / 0.25 / 0.75; row 2: own bin, no runner-up (+inf margins);
    # row 1: margin 0 at one entry and another bin at the last; rows 3, 4: another bin at one entry;
    # rows 5 .. 7: no label in [0, 3) -- row 5's bin -1 "equals" its own -1 at two entries and still does not count
    assert np.array_equal(s.stable(), [True, False, True, False, False, False, False, False])
    assert s.stable().dtype == np.bool_
    assert np.array_equal(s.stable(0.25), [False, False, True, False, False, False, False, False])   # (above, not at)
    assert np.array_equal(s.stable(0.2), s.stable())
    assert np.array_equal(s.stable(1e300), [False, False, True, False, False, False, False, False])
    assert s.distances is None


def test_bound_and_exported():
    import chbin_amd
    lib = _lib.load()
    for name in ("chb_audit_rows_multi", "chb_recruit_rows_multi"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["chb_audit_rows_multi"][1]) == 11 and len(_lib.SIGNATURES["chb_recruit_rows_multi"][1]) == 12
    assert chbin_amd.neighbor_sweep is clustering.neighbor_sweep and "neighbor_sweep" in chbin_amd.__all__
    assert callable(_lib.Context.audit_rows_multi) and callable(_lib.Context.recruit_rows_multi)
    fields = [f.name for f in __import__("dataclasses").fields(clustering.NeighborSweep)]
    for name in ("neighbors", "rows", "own", "bins", "min_dist", "margin", "distances"):
        assert name in fields


def test_no_cpu_fallback():
    """Without a GPU the call fails loudly, as the other mirrors do."""
    if _lib.load().chb_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep(np.zeros((4, 4)), np.zeros(4, dtype=np.int64), 1)
    with pytest.raises(_lib.ChbError):
        clustering.neighbor_sweep(np.zeros((4, 4)), np.zeros(4, dtype=np.int64), 1, neighbors=(2, 1), rows=np.array([0]))
