"""Leave-group-out audit without a device: clustering.parent_groups, the numpy statement of the withheld set W(r) that the
GPU tests build their yardstick from (groups_reference.py), the GPU tests' data set, and the Python surface."""
import inspect

import numpy as np
import pytest

import groups_reference as G


def test_parent_groups_codes_by_first_occurrence():
    from chbin_amd import clustering
    names = ["k141_7", "k141_2", "k141_7", "k141_9", "k141_2", "k141_7"]
    got = clustering.parent_groups(names)
    assert got.dtype == np.int64 and got.shape == (6,)
    assert got.tolist() == [0, 1, 0, 2, 1, 0]
    # equal names give equal codes and different names different ones, whatever the container
    again = clustering.parent_groups(np.array(names, dtype=object))
    assert np.array_equal(got, again)
    assert clustering.parent_groups([]).shape == (0,) and clustering.parent_groups([]).dtype == np.int64
    assert clustering.parent_groups(["a"]).tolist() == [0]
    many = [f"c{i % 50}" for i in range(500)]
    codes = clustering.parent_groups(many)
    assert codes.min() == 0 and codes.max() == 49 and np.array_equal(codes, np.arange(500) % 50)


def test_withheld_set_on_a_hand_made_case():
    #                 0   1   2      3   4      5   6   7
    groups = np.array([5, -1, 2 ** 62, 5, -1, 2 ** 62, -3, 5], dtype=np.int64)
    assert G.withheld(groups, 0).tolist() == [0, 3, 7]
    assert G.withheld(groups, 3).tolist() == [0, 3, 7]
    assert G.withheld(groups, 2).tolist() == [2, 5]
    # negative ids are not groups: equal negative values withhold nothing but the row
    assert G.withheld(groups, 1).tolist() == [1]
    assert G.withheld(groups, 4).tolist() == [4]
    assert G.withheld(groups, 6).tolist() == [6]
    labels = np.array([0, 0, 1, 1, 0, 9, -1, 0], dtype=np.int64)
    # siblings go whatever their label (row 3 sits in bin 1), nothing else moves, the input is left alone
    assert G.labels_without(labels, groups, 0).tolist() == [-1, 0, 1, -1, 0, 9, -1, -1]
    assert G.labels_without(labels, groups, 4).tolist() == [0, 0, 1, 1, -1, 9, -1, 0]
    assert labels.tolist() == [0, 0, 1, 1, 0, 9, -1, 0]
    # all rows without a group, and all rows in groups of their own: W(r) = {r}
    for g in (np.full(8, -1), np.arange(8)):
        assert all(G.withheld(g, r).tolist() == [r] for r in range(8))


def test_gpu_data_set_has_every_edge():
    X, labels, groups = G.group_data()
    assert X.shape == (G.N, G.D) and labels.shape == groups.shape == (G.N,)
    inside = (labels >= 0) & (labels < G.B)
    assert 30 <= np.count_nonzero(~inside) <= 50 and (labels == -1).any() and (labels >= G.B).any() and (labels < -1).any()
    sizes = {int(g): int(np.count_nonzero(groups == g)) for g in np.unique(groups[groups >= 0])}
    assert {1, 2, 4, 70} <= set(sizes.values())
    assert {0, 7, 2 ** 40 + 3, 2 ** 62} <= set(sizes)
    big = groups == G.BIG
    assert sizes[G.BIG] == 70 and set(labels[big].tolist()) == {0, 1}
    # one group holds every member of a bin, one leaves a bin fewer than five
    assert np.all(groups[labels == G.SMALL_BIN] == G.ALL_OF_BIN) and np.count_nonzero(labels == G.SMALL_BIN) == 6
    left = np.count_nonzero((labels == G.STARVED_BIN) & (groups != G.STARVER))
    assert 0 < left < 5
    # a pair of twins in one group and a twin outside it
    tw = np.flatnonzero((groups == G.TWINS) & (labels == 0))
    assert len(tw) == 2 and np.array_equal(X[tw[0]], X[tw[1]])
    same = np.flatnonzero((X == X[tw[0]]).all(axis=1))
    assert len(same) == 3 and np.count_nonzero(groups[same] == G.TWINS) == 2 and np.all(labels[same] == 0)
    # a third of the rows without a group, under several negative values
    neg = groups < 0
    assert G.N // 3 - 5 <= np.count_nonzero(neg) <= G.N // 3 + 5 and len(np.unique(groups[neg])) >= 3
    # scattered: the four rows of a thread and the 64 of a tile mix groups and ungrouped rows
    quads = groups.reshape(-1, 4)
    mixed = sum(1 for q in quads if (q < 0).any() and (q >= 0).any() and len(set(q.tolist())) >= 3)
    assert mixed > len(quads) // 3
    for t in groups.reshape(-1, 64):
        assert (t < 0).any() and len(np.unique(t[t >= 0])) >= 10
    assert np.count_nonzero(big.reshape(-1, 64).any(axis=1)) >= 8   # the large group reaches most query tiles
    assert (~inside & (groups >= 0)).any() and (~inside & neg).any()   # unlabelled rows with and without siblings


@pytest.mark.parametrize("name", ["audit", "bin_report", "neighbor_sweep", "audit_pairs", "cohesion"])
def test_groups_is_the_last_keyword(name):
    from chbin_amd import clustering
    params = list(inspect.signature(getattr(clustering, name)).parameters.values())
    assert params[-1].name == "groups" and params[-1].default is None


def test_bindings_take_groups_after_labels():
    from chbin_amd import _lib
    pairs = {"chb_audit_rows": "chb_audit_rows_grouped", "chb_audit_rows_multi": "chb_audit_rows_multi_grouped",
             "chb_audit_pairs": "chb_audit_pairs_grouped", "chb_bin_report": "chb_bin_report_grouped"}
    for plain, grouped in pairs.items():
        res, args = _lib.SIGNATURES[plain]
        gres, gargs = _lib.SIGNATURES[grouped]
        assert gres is res and len(gargs) == len(args) + 1
        assert gargs[:2] == args[:2] and gargs[3:] == args[2:]   # context, labels, GROUPS, the rest
    assert not any(n.startswith("chb_recruit") and n.endswith("_grouped") for n in _lib.SIGNATURES)
