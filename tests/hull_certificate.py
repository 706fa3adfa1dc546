"""A hull-distance reference that certifies itself, for vertex sets no other yardstick of this suite covers: more than 16
vertices that are exactly dependent (duplicates, one-hot rows, more vertices than dimensions) and badly scaled.

row_reference.py leaves the distance of 13 and more vertices to the oracle's Goldfarb-Idnani, which goes through
nearest_positive_definite on a singular Gram and is good to about 1e-8 there; chb_hull_distance_batch is the driver under
test on another Gram arithmetic.  Here the distance comes with a proof instead of a pedigree.  For vertices y_i (shifted
to the scored row, so the query is the origin) and ANY feasible weights alpha (>= 0, sum 1), with z = alpha @ Y:

    hi = ||z||                          z is a point of the hull: the distance is at most hi
    lo = max(0, min_i <y_i, z> / ||z||)   every hull point p has <p, z> >= min_i <y_i, z>, so ||p|| >= lo

Both are evaluated in np.longdouble from the weights alone.  The true distance lies in [lo, hi] whatever produced alpha:
the solver (min_norm_point: Wolfe's active-set method in fp64, plain numpy) does not have to be trusted, only the width of
its bracket checked -- test_hull_certificate_cpu.py asserts hi - lo <= 1e-10 of the scale on every problem the GPU tests
use.  Nearly dependent sets (thin slabs) are not what this is for: the solver does not close the bracket on them.

Selection is row_reference's: oracle.cdist_row, the row itself withheld for an audit, oracle.find_nearest_from_cluster."""
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# lo, hi, scale [n, B] (an empty bin: lo = hi = +inf, scale 0); sets: per row a list of B index arrays, (distance, index) order
Certified = namedtuple("Certified", "lo hi scale sets")

LD = np.longdouble


def _pow2_below(v):
    """the power of two p with p <= v < 2 p (v > 0, finite): scaling by it is exact"""
    return np.ldexp(1.0, int(np.frexp(float(v))[1]) - 1)


def min_norm_point(Yshift, max_major=400):
    """Feasible weights [n] (>= 0, sum 1) of a point of conv(Yshift) close to the one of least norm: Wolfe's method.  The
    affine minimiser on the support solves the bordered system [[0, 1^T], [1, G_SS]] (mu, b) = (1, 0) by lstsq, so
    duplicated vertices are harmless; G is the Gram normalised by the largest squared norm.  The gradient and the
    objective are evaluated on the points themselves, not on the Gram: inside the hull the Gram's form loses z at the
    root of the rounding error."""
    Y = np.ascontiguousarray(Yshift, dtype=np.float64)
    n = len(Y)
    nrm2 = (Y * Y).sum(axis=1)
    if n == 1 or not nrm2.max() > 0.0:
        w = np.zeros(n)
        w[int(np.argmin(nrm2))] = 1.0
        return w
    P = Y / _pow2_below(np.sqrt(nrm2.max()))   # (largest norm in [1, 2))
    G = P @ P.T
    G /= G.diagonal().max()
    w = np.zeros(n)
    w[int(np.argmin(G.diagonal()))] = 1.0
    S = w > 0.0
    best_w, best_gap = w.copy(), np.inf
    for _ in range(max_major):
        z = w @ P
        val = z @ z
        g = P @ z
        gap = val - g.min()
        if gap < best_gap:
            best_w, best_gap = w.copy(), gap
        j = int(np.argmin(g))
        if S[j] or not g[j] < val - 1e-16 * max(val, 1e-300) - 1e-30:
            break
        S[j] = True
        for _ in range(n + 1):
            idx = np.flatnonzero(S)
            k = len(idx)
            A = np.empty((k + 1, k + 1))
            A[0, 0] = 0.0
            A[0, 1:] = 1.0
            A[1:, 0] = 1.0
            A[1:, 1:] = G[np.ix_(idx, idx)]
            rhs = np.zeros(k + 1)
            rhs[0] = 1.0
            b = np.linalg.lstsq(A, rhs, rcond=None)[0][1:]
            b = b / b.sum()
            if np.all(b > 0.0):
                w[:] = 0.0
                w[idx] = b
                break
            ws = w[idx]
            den = ws - b
            bad = b <= 0.0
            theta = np.where(bad & (den > 0.0), ws / np.where(den > 0.0, den, 1.0), np.inf)
            theta[bad & ~(den > 0.0)] = 0.0
            r = int(np.argmin(theta))
            t = min(1.0, float(theta[r]))
            ws = ws + t * (b - ws)
            ws[r] = 0.0
            ws[ws < 0.0] = 0.0
            w[:] = 0.0
            w[idx] = ws / ws.sum()
            S[idx[r]] = False
            S &= w > 0.0
            if not S.any():   # (cannot happen with exact arithmetic; keep the best point seen)
                w = best_w.copy()
                S = w > 0.0
                break
    z = w @ P
    g = P @ z
    if z @ z - g.min() < best_gap:
        best_w = w
    w = np.maximum(best_w, 0.0)
    return w / w.sum()


def bracket(Yshift, alpha):
    """(lo, hi, scale) of the distance from the origin to conv(Yshift), from feasible weights alone, in np.longdouble
    (returned as float64, lo rounded down and hi up by one ulp); scale = max_i ||y_i|| as row_reference computes it."""
    Y = np.ascontiguousarray(Yshift, dtype=np.float64)
    scale = float(np.sqrt((Y * Y).sum(axis=1)).max())
    if scale == 0.0:
        return 0.0, 0.0, 0.0
    a = np.asarray(alpha, dtype=np.float64)
    assert a.shape == (len(Y),) and np.all(a >= 0.0) and abs(a.sum() - 1.0) < 1e-9
    p2 = _pow2_below(scale)
    Yl = Y.astype(LD) / LD(p2)
    al = a.astype(LD)
    al = al / al.sum()
    z = al @ Yl
    nz = np.sqrt(z @ z)
    if nz == 0:   # (the origin itself: a vertex with weight 1, or an exact cancellation)
        return 0.0, 0.0, scale
    hi = float(np.nextafter(float(nz) * p2, np.inf))
    lo = float((Yl @ z).min() / nz) * p2
    lo = max(0.0, float(np.nextafter(lo, -np.inf)))
    return lo, hi, scale


def affine_distance(Yshift):
    """Distance from the origin to the affine hull of the rows of Yshift, by lstsq on P[1:] - P[0]; for affinely
    independent sets (the residual of a rank-deficient system is still right, but nothing here needs it)."""
    Y = np.ascontiguousarray(Yshift, dtype=np.float64)
    nrm = np.sqrt((Y * Y).sum(axis=1)).max()
    if not nrm > 0.0:
        return 0.0
    p2 = _pow2_below(nrm)
    P = Y / p2
    if len(P) == 1:
        return float(np.sqrt(P[0] @ P[0])) * p2
    E = (P[1:] - P[0]).T
    c = np.linalg.lstsq(E, -P[0], rcond=None)[0]
    r = P[0] + E @ c
    return float(np.sqrt(r @ r)) * p2


def _select(args):
    from oracle import oracle as O
    Z, labels, i, own, B, m = args
    row = O.cdist_row(Z, i)[:len(labels)]
    lab = labels
    if own is not None:   # audit: withhold the row itself and nothing else
        lab = labels.copy()
        lab[own] = -1
    return [O.find_nearest_from_cluster(c, lab, row, m) for c in range(B)]


def _jobs(X, labels, B, m, Y, rows):
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    N = len(X)
    if Y is not None:
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        Z = np.ascontiguousarray(np.vstack([X, Y]))
        rows = np.arange(len(Y)) if rows is None else np.asarray(rows)
        return X, [Y[int(q)] for q in rows], [(Z, labels, N + int(q), None, B, m) for q in rows]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    return X, [X[int(r)] for r in rows], [(X, labels, int(r), int(r), B, m) for r in rows]


def _pool():
    return ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))


def selected_sets(X, labels, B, m, Y=None, rows=None):
    """Per scored row the B selected index arrays, exactly as row_reference._one_row selects them.  (The order is
    (distance, index), so the sets of a smaller m are the leading entries of these.)"""
    _, _, jobs = _jobs(X, labels, B, m, Y, rows)
    with _pool() as pool:   # (the oracle is a ctypes library: each call drops the GIL)
        return list(pool.map(_select, jobs))


def padded(sets, B, m):
    """[rows, B, m] int64: the leading m entries of every set, -1 padded -- the layout of topm_per_bin's nbr_idx"""
    out = np.full((len(sets), B, m), -1, dtype=np.int64)
    for q, per_bin in enumerate(sets):
        for c, idx in enumerate(per_bin):
            k = min(m, len(idx))
            out[q, c, :k] = idx[:k]
    return out


def certified_rows(X, labels, B, m, Y=None, rows=None, sets=None):
    """The bracket of every (row, bin) hull distance as a Certified.  Y given (recruit): the rows Y[rows], nothing
    withheld; Y None (audit): the resident rows X[rows], each withheld from its own candidates.  sets: selected_sets of
    the same rows at this m or a larger one, if the caller has them already."""
    X, xs, jobs = _jobs(X, labels, B, m, Y, rows)
    if sets is None:
        with _pool() as pool:
            sets = list(pool.map(_select, jobs))
    sets = [[idx[:m] for idx in per_bin] for per_bin in sets]

    def one(k):
        lo, hi, scale = np.full(B, np.inf), np.full(B, np.inf), np.zeros(B)
        for c in range(B):
            idx = sets[k][c]
            if len(idx) == 0:
                continue
            P = X[idx] - xs[k]
            lo[c], hi[c], scale[c] = bracket(P, min_norm_point(P))
        return lo, hi, scale

    with _pool() as pool:
        out = list(pool.map(one, range(len(xs))))
    lo, hi, scale = (np.array([o[i] for o in out]).reshape(len(xs), B) for i in range(3))
    for a in (lo, hi, scale):
        a.setflags(write=False)
    return Certified(lo, hi, scale, sets)


def as_reference(cert):
    """The bracket's midpoint as a row_reference.RowReference, for bound() and clear_rows()"""
    from row_reference import RowReference
    with np.errstate(invalid="ignore"):
        mid = np.where(np.isfinite(cert.hi), 0.5 * (cert.lo + cert.hi), np.inf)
    return RowReference(mid, cert.scale, cert.sets)
