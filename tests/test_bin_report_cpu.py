"""clustering.BinReport's pure-numpy helpers on hand-made tables, and bin_report without a device (no GPU needed)."""
import numpy as np
import pytest

from chbin_amd import _lib, clustering


def make_report():
    confusion = np.array([[90, 6, 2, 0],
                          [10, 30, 0, 10],
                          [0, 0, 0, 0],
                          [1, 1, 1, 5]], dtype=np.int64)
    unplaced = np.array([2, 0, 0, 2], dtype=np.int64)
    dcnt = np.array([[100, 100, 100, 0],
                     [50, 49, 50, 0],
                     [0, 0, 0, 0],
                     [10, 10, 10, 0]], dtype=np.int64)
    dsum = np.where(dcnt > 0, dcnt * np.array([[0.5], [0.25], [1.0], [2.0]]), 0.0)
    dmin = np.where(dcnt > 0, 0.125, np.inf)
    return clustering.BinReport(confusion, unplaced, dcnt, dmin, dsum, 7)


def test_mean_is_nan_exactly_where_nothing_was_counted():
    r = make_report()
    mean = r.mean
    assert mean.shape == (4, 4) and mean.dtype == np.float64
    assert np.array_equal(np.isnan(mean), r.dcnt == 0)
    assert np.array_equal(mean[0, :3], [0.5, 0.5, 0.5]) and np.array_equal(mean[1, :3], [0.25, 0.25, 0.25])
    assert np.array_equal(mean[3, :3], [2.0, 2.0, 2.0])
    assert np.array_equal(r.dsum, make_report().dsum)   # (the tables themselves are left alone)


def test_confused_pairs_order_and_threshold():
    r = make_report()
    # shares: bin 0 has 100 rows (2 unplaced), bin 1 has 50, bin 2 none, bin 3 has 10 (2 unplaced)
    assert r.confused_pairs(0.0) == [(1, 0, 0.2), (1, 3, 0.2), (3, 0, 0.1), (3, 1, 0.1), (3, 2, 0.1), (0, 1, 0.06), (0, 2, 0.02)]
    assert r.confused_pairs(0.1) == [(1, 0, 0.2), (1, 3, 0.2), (3, 0, 0.1), (3, 1, 0.1), (3, 2, 0.1)]
    assert r.confused_pairs(0.06) == r.confused_pairs(0.1) + [(0, 1, 0.06)]   # (the threshold itself counts)
    assert r.confused_pairs(0.21) == []
    assert r.confused_pairs() == r.confused_pairs(0.05)
    for a, b, share in r.confused_pairs(0.0):
        assert a != b and isinstance(a, int) and isinstance(b, int) and isinstance(share, float)


def test_bound_and_exported():
    import chbin_amd
    assert "chb_bin_report" in _lib.SIGNATURES and hasattr(_lib.load(), "chb_bin_report")
    assert chbin_amd.bin_report is clustering.bin_report and "bin_report" in chbin_amd.__all__
    assert callable(_lib.Context.bin_report)


def test_no_cpu_fallback():
    """Without a GPU the call fails loudly, as the other mirrors do."""
    if _lib.load().chb_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.ChbError):
        clustering.bin_report(np.zeros((4, 4)), np.zeros(4, dtype=np.int64), 1)
    # (the C call itself needs a context, and chb_create is what reports CHB_ENODEVICE)
    with pytest.raises(_lib.ChbError, match="-2|no HIP device"):
        _lib.Context(0)
