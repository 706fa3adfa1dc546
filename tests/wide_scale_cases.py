"""The data of the wide row-scoring tests on ill-scaled, tied and odd-width data (test_hull_certificate_cpu.py,
test_gpu_wide_m_scales.py), and their certified references (hull_certificate.py), computed once per process.

Scale axis: test_gpu_row_scoring_scales.case_data's deformations -- offset 1000, 1e-50, 1e+50, log-normal column scales,
one 1e6 outlier, bins 1e3 apart, 150 equal members, one-hot rows -- at N = 600, D = 136 (onehot: 24), B = 4, Q = 130,
with lists of 17, 32, 33 and 64 members: either side of the hull_wide_kernel<32> / <64> split and the full list.  About
105 members per bin keep the m = 64 lists full; bin SMALL is cut to 20 members, so hull_wide_kernel<64> also runs with two
of its four 16-vertex blocks empty.

Width axis: wide_m_cases' friendly data (centre + 0.3 normal) at N = 400, B = 4, bins of 0, 20, 70 and 310 members,
Q = 70, at every feature width on an edge of hull_wide_kernel's 16-feature step: a single step with idle lane quarters
(1, 2, 7, 8), a padded width that is a multiple of 16 (9 -> 16, 16, 32), one past it (17, 33), the benchmark's 136 and
long rows of 19 and 38 steps (300, 600)."""
import functools

import numpy as np

import hull_certificate as H
import test_gpu_row_scoring_scales as S

KINDS = S.KINDS
EXEMPT = S.EXEMPT
N, B, Q = S.N, 4, 130
MS = (17, 32, 33, 64)
SMALL, N_SMALL = 3, 20    # the bin that is cut down, and what is left of it

# rseed draws the labels and the deformation (S.case_data), chosen per kind so that the tie rule's cap holds by the
# reference alone (test_hull_certificate_cpu.py)
RSEED = {k: 7 for k in KINDS}

# The deformations live in S.case_data, which reads its parameters from S.CASES by name: the wide cases are entered there
# under names of their own (S.NAMES, the list S's own tests run over, was taken before and does not see them).  m = 64
# only seeds the generator; the lists are cut per test.
for _k in KINDS:
    S.CASES.setdefault(f"{_k}_wide64", dict(kind=_k, D=24 if _k == "onehot" else 136, B=B, m=64, Q=Q, rseed=RSEED[_k]))


def dim(kind):
    return S.CASES[f"{kind}_wide64"]["D"]


@functools.lru_cache(maxsize=None)
def case_data(kind):
    """(X, labels, Y, rows, copies): S.case_data's draw of the kind with bin SMALL cut to N_SMALL members drawn at
    random; rows = every sixth resident row and every member of bin SMALL; copies as there: None, or for `identical`
    (positions in Y, positions in rows) of the scored rows that are copies of the 150 equal members of bin 0."""
    X, labels, Y, _, copies = S.case_data(f"{kind}_wide64")
    labels = labels.copy()
    members = np.flatnonzero(labels == SMALL)
    keep = np.random.default_rng(11).choice(members, N_SMALL, replace=False)
    labels[np.setdiff1d(members, keep)] = -1
    rows = np.unique(np.concatenate([np.arange(0, N, 6), keep])).astype(np.int64)
    if copies is not None:
        equal = np.flatnonzero((X == Y[copies[0][0]]).all(axis=1) & (labels == 0))
        copies = (copies[0], np.flatnonzero(np.isin(rows, equal)))
    for a in (labels, rows):
        a.setflags(write=False)
    return X, labels, Y, rows, copies


@functools.lru_cache(maxsize=None)
def case_sets(kind, call):
    """selected_sets at m = 64 of the scored rows of a call ("recruit": all of Y, "audit": rows)"""
    X, labels, Y, rows, _ = case_data(kind)
    if call == "recruit":
        return H.selected_sets(X, labels, B, 64, Y=Y)
    return H.selected_sets(X, labels, B, 64, rows=rows)


@functools.lru_cache(maxsize=None)
def case_certificate(kind, call, m):
    X, labels, Y, rows, _ = case_data(kind)
    if call == "recruit":
        return H.certified_rows(X, labels, B, m, Y=Y, sets=case_sets(kind, call))
    return H.certified_rows(X, labels, B, m, rows=rows, sets=case_sets(kind, call))


@functools.lru_cache(maxsize=None)
def grid_sets(kind):
    """selected_sets at m = 64 of the audit of EVERY resident row, and of all of Y: the selection tests' whole grid"""
    X, labels, Y, _, _ = case_data(kind)
    return H.selected_sets(X, labels, B, 64), case_sets(kind, "recruit")


# ---- the width axis

WN, WQ = 400, 70
WSIZES = (0, 20, 70, 310)
WIDTHS = (1, 2, 7, 8, 9, 16, 17, 32, 33, 136, 300, 600)
WMS = (17, 64)
# In one or two dimensions the hulls of 17 and more members of overlapping clusters contain most rows of the other bins:
# zeros in several bins are the construction, as in `identical` and `onehot`, and these widths are exempt from the cap the
# same way (the chosen bin's reference distance must then be within the bound of the reference minimum).
WEXEMPT = (1, 2)


@functools.lru_cache(maxsize=None)
def width_data(D, seed=5):
    """(X [WN, D], labels, Y [WQ, D], rows): wide_m_cases.wide's draw at these sizes; rows = every fourth resident row and
    every member of the 20-member bin"""
    assert sum(WSIZES) == WN
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(B), WSIZES)).astype(np.int64)
    cen = rng.normal(size=(B, D))
    X = np.ascontiguousarray(cen[lab] + 0.3 * rng.normal(size=(WN, D)))
    Y = np.ascontiguousarray(cen[rng.integers(1, B, WQ)] + 0.3 * rng.normal(size=(WQ, D)))
    rows = np.unique(np.concatenate([np.arange(0, WN, 4), np.flatnonzero(lab == 1)])).astype(np.int64)
    for a in (X, lab, Y, rows):
        a.setflags(write=False)
    return X, lab, Y, rows


@functools.lru_cache(maxsize=None)
def width_sets(D, call):
    X, lab, Y, rows = width_data(D)
    if call == "recruit":
        return H.selected_sets(X, lab, B, 64, Y=Y)
    return H.selected_sets(X, lab, B, 64, rows=rows)


@functools.lru_cache(maxsize=None)
def width_certificate(D, call, m):
    X, lab, Y, rows = width_data(D)
    if call == "recruit":
        return H.certified_rows(X, lab, B, m, Y=Y, sets=width_sets(D, call))
    return H.certified_rows(X, lab, B, m, rows=rows, sets=width_sets(D, call))


@functools.lru_cache(maxsize=None)
def width_grid_sets(D):
    X, lab, Y, _ = width_data(D)
    return H.selected_sets(X, lab, B, 64), width_sets(D, "recruit")


def closed_form_1d(x, p):
    """the distance of the number x to the hull [min p, max p] of the numbers p"""
    return max(0.0, float(p.min() - x), float(x - p.max()))
