"""A reference for the row-scoring entry points (chb_recruit_rows, chb_audit_rows and their list, pair and report forms)
that depends neither on the origin nor on the scale of the data.

The suite's older yardstick for these calls, oracle.sweep(..., want_all=True), solves the reference project's own QP form
2 P P^T on the UNSHIFTED vertices: on data with a common offset, or far from unit scale, that form loses the answer (the
TINY comment of test_gpu_bin_distances.py; kind 5 of test_hull_distance_16_lane_solver_both_starts).  Here the two steps
are taken apart:

  selection  the oracle's own: oracle.cdist_row from the scored row (the k-sequential unfused sum of squared differences,
             the arithmetic the kernels' selection is documented to share bit for bit), the row's own label set to -1 for
             an audit (leave-one-out: only the row itself, a twin stays), then oracle.find_nearest_from_cluster per bin
             -- the (distance, index) order.  The selected index SET is therefore exact.
  distance   of the selected vertices P to the row x on the problem shifted to the row, which does not depend on the
             origin: oracle.enum_hull_distance(0, P - x) up to 12 vertices (exhaustive, no pivoting order), and for 13 to
             16 oracle.convex_hull_distance(0, P - x), Goldfarb-Idnani on the shifted Gram -- the two yardsticks
             test_gpu_parity.py uses for the stand-alone solver.  Both normalise by the problem's own largest entry, so a
             power-of-two scaling of the data scales the answer exactly.  An empty bin gives +inf.

Every entry comes with scale = max_i ||p_i - x||, the unit of the relative envelope below."""
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# dist [n, B], scale [n, B] (0 for an empty bin), sets: per row a list of B index arrays in (distance, index) order, or None
RowReference = namedtuple("RowReference", "dist scale sets")

ENUM_MAX = 12   # the enumerator's limit in this suite (2^12 supports per problem)
REL_TOL = 1e-9          # of the scale: the envelope test_hull_distance_16_lane_solver_both_starts asserts
ZERO_TOL = 1e-7         # ... and its allowance for a distance of zero, the root of a rounding-sized square
ZERO_BELOW = 1e-6       # ... which applies below this fraction of the scale


def _one_row(args):
    from oracle import oracle as O
    Z, labels, i, own, x, X, B, m = args
    row = O.cdist_row(Z, i)[:len(labels)]
    lab = labels
    if own is not None:   # audit: withhold the row itself and nothing else
        lab = labels.copy()
        lab[own] = -1
    D = X.shape[1]
    zero = np.zeros(D)
    dist, scale, sets = np.full(B, np.inf), np.zeros(B), []
    for c in range(B):
        idx = O.find_nearest_from_cluster(c, lab, row, m)
        sets.append(idx)
        if len(idx) == 0:
            continue
        P = np.ascontiguousarray(X[idx] - x)
        scale[c] = np.sqrt((P * P).sum(axis=1)).max()
        if scale[c] == 0.0:   # every vertex is the row itself: 0 by definition, whatever the solver makes of a zero Gram
            dist[c] = 0.0
        elif len(idx) <= ENUM_MAX:
            dist[c] = O.enum_hull_distance(zero, P)
        else:
            dist[c] = O.convex_hull_distance(zero, P)
    return dist, scale, sets


def reference_rows(X, labels, B, m, *, Y=None, rows=None, want_sets=False):
    """Hull distances [n, B] (float64) of rows to every bin of the frozen `labels`, with their scales and, on request, the
    selected index sets, as a RowReference.

    Y given (recruit): the rows Y[rows] (rows=None: all of Y), which are not samples; nothing is withheld.
    Y None (audit): the resident rows X[rows] (rows=None: all of them), each withheld from its own candidates."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    N = len(X)
    if Y is not None:
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        Z = np.ascontiguousarray(np.vstack([X, Y]))
        rows = np.arange(len(Y)) if rows is None else np.asarray(rows)
        jobs = [(Z, labels, N + int(q), None, Y[int(q)], X, B, m) for q in rows]
    else:
        rows = np.arange(N) if rows is None else np.asarray(rows)
        jobs = [(X, labels, int(r), int(r), X[int(r)], X, B, m) for r in rows]
    # (the oracle is a ctypes library: each call drops the GIL)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        out = list(pool.map(_one_row, jobs))
    dist = np.array([o[0] for o in out]).reshape(len(rows), B)
    scale = np.array([o[1] for o in out]).reshape(len(rows), B)
    for a in (dist, scale):
        a.setflags(write=False)
    return RowReference(dist, scale, [o[2] for o in out] if want_sets else None)


def bound(ref):
    """[n, B] the largest |d - ref.dist| a finite entry may show: 1e-9 of the scale, and 1e-7 of it more where the reference
    distance is below 1e-6 of the scale (0 for an empty bin)."""
    with np.errstate(invalid="ignore"):
        near_zero = ref.dist < ZERO_BELOW * ref.scale
    return REL_TOL * ref.scale + ZERO_TOL * ref.scale * near_zero


def strict_argmin(dist):
    """(bin, runner-up bin) of every row by the reference's strict-'>' scan: lowest index among equal minima, -1 when every
    entry is +inf; the runner-up is the lowest index among the smallest other entries, -1 without a finite one."""
    n, B = dist.shape
    best, second = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for q in range(n):
        d = dist[q]
        fin = np.flatnonzero(np.isfinite(d))
        if len(fin) == 0:
            continue
        best[q] = fin[np.argmin(d[fin])]
        rest = fin[fin != best[q]]
        if len(rest):
            second[q] = rest[np.argmin(d[rest])]
    return best, second


def clear_rows(ref):
    """(bin [n], clear [n]): the reference's bin of every row, and whether its margin to the runner-up exceeds twice the
    bound of its two best entries -- only then must a result within the bound choose the same bin.  A row without a
    runner-up is clear."""
    best, second = strict_argmin(ref.dist)
    b = bound(ref)
    q = np.arange(len(best))
    has2 = second >= 0
    margin = np.where(has2, ref.dist[q, np.maximum(second, 0)] - ref.dist[q, np.maximum(best, 0)], np.inf)
    thr = 2.0 * np.maximum(b[q, np.maximum(best, 0)], b[q, np.maximum(second, 0)])
    return best, ~has2 | (margin > thr)
