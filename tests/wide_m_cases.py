"""The data of the wide-m tests (test_wide_m_cpu.py, test_gpu_wide_m.py): a labelling with a bin on every edge of the wide
kernels -- no member, one, the old list limit of 16, just past it, and either side of the 64-member tile and of the
64-entry list -- and its oracle references, computed once per process."""
import functools

import numpy as np

import row_reference

N, B, Q = 700, 8, 200
SIZES = (0, 1, 16, 17, 63, 64, 65, 474)   # members of bin 0 .. 7


@functools.lru_cache(maxsize=None)
def wide(D, seed=5, twins=0):
    """(X [N, D], labels [N], Y [Q, D], twin pairs [(copy, source)]): X = cen[lab] + 0.3 normal around centres drawn from
    normal(B, D), the labels a permutation of SIZES' runs; with `twins` that many rows are overwritten by copies of that
    many others (they keep their own labels).  Y: Q rows drawn the same way around random centres."""
    assert sum(SIZES) == N
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(B), SIZES)).astype(np.int64)
    cen = rng.normal(size=(B, D))
    X = cen[lab] + 0.3 * rng.normal(size=(N, D))
    pairs = []
    if twins:
        pick = rng.permutation(N)[: 2 * twins]
        for t, s in zip(pick[:twins], pick[twins:]):
            X[t] = X[s]
            pairs.append((int(t), int(s)))
    Y = cen[rng.integers(1, B, Q)] + 0.3 * rng.normal(size=(Q, D))
    for a in (X, lab, Y):
        a.setflags(write=False)
    return np.ascontiguousarray(X), lab, np.ascontiguousarray(Y), tuple(pairs)


def oracle_rows(m):
    """The resident rows the oracle checks score at this m: all of them at m = 17, else every seventh and the members of the
    bins of size 1, 16 and 17 (D does not matter: the labels of a seed are the same)."""
    lab = wide(72)[1]
    if m == 17:
        return np.arange(N, dtype=np.int64)
    small = np.flatnonzero((lab == 1) | (lab == 2) | (lab == 3))
    return np.unique(np.concatenate([np.arange(0, N, 7), small])).astype(np.int64)


@functools.lru_cache(maxsize=None)
def audit_reference(D, m, twins, every_seventh=False):
    X, lab, _, _ = wide(D, twins=twins)
    rows = np.arange(0, N, 7, dtype=np.int64) if every_seventh else oracle_rows(m)
    return rows, row_reference.reference_rows(X, lab, B, m, rows=rows, want_sets=True)


YROWS = np.arange(0, Q, 4)   # the rows of Y the oracle scores (the calls score all of Y)


@functools.lru_cache(maxsize=None)
def recruit_reference(D, m, twins):
    X, lab, Y, _ = wide(D, twins=twins)
    return row_reference.reference_rows(X, lab, B, m, Y=Y, rows=YROWS, want_sets=True)


def padded_sets(sets, m):
    """[rows, B, m] int64: the reference's index sets, -1 padded -- the layout of topm_per_bin's nbr_idx"""
    out = np.full((len(sets), B, m), -1, dtype=np.int64)
    for q, per_bin in enumerate(sets):
        for c, idx in enumerate(per_bin):
            out[q, c, : len(idx)] = idx
    return out
