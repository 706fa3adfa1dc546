#!/usr/bin/env python3
"""How many affine solves the per-lane Wolfe solver (min_norm_point<M> in qp_kernels.hip, m <= 8) needs per problem, from
the nearest vertex and from the full vertex set, counted on the CPU (numpy only).

A replica of the solver -- the same major / minor cycles, the same lifted LDL^T with its pivot test, the same tolerances --
runs both starts on hull problems of the benchmark's generator: true labels as members, a sample of queries x every bin,
the m nearest members of each.  It prints the histogram of the final support's size, the solves per problem, and the
solves a wavefront pays for -- the maximum over the 64 problems it holds, in both work orders of the fused kernel: one
position x 64 bins, and the striped 8 positions x the 8 bins of one XCD (fused_pair_of).

usage: tools/solver_start_probe.py [--contigs N] [--dim D] [--bins B] [--neighbors m] [--queries k]
       (the default generator and the two `extra` generators of bench.py, one table each)
"""
import argparse
import importlib.util
import os

import numpy as np

GENERATORS = (("default", 0.0, 1.5e-3), ("overlapping_bins", 0.3, 4.5e-3), ("collapsed_bins", 0.5, 6e-3))


def load_synth():
    """ch-bin_amd/synth.py without importing the package (which loads the GPU library)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("chb_synth", os.path.join(root, "ch-bin_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def solve_affine(Q, s, S):
    """solve_affine<M>: (Q_SS + s 11^T) b = 1 by LDL^T without pivoting, beta = b / sum(b); False when a pivot collapses."""
    idx = np.flatnonzero(S)
    n = len(idx)
    A = Q[np.ix_(idx, idx)] + s
    L = np.eye(n)
    d = np.zeros(n)
    for k in range(n):
        d[k] = A[k, k] - (L[k, :k] ** 2) @ d[:k]
        if not d[k] > 1e-13 * A[k, k]:
            return False, None
        for i in range(k + 1, n):
            L[i, k] = (A[i, k] - (L[i, :k] * L[k, :k]) @ d[:k]) / d[k]
    z = np.linalg.solve(L, np.ones(n)) / d
    b = np.linalg.solve(L.T, z)
    beta = np.zeros(len(Q))
    beta[idx] = b / b.sum()
    return bool(b.sum() > 0.0), beta


def min_norm_point(Q, full_start):
    """min_norm_point<M> on the m x m Gram Q.  Returns (value, weights, support mask, affine solves)."""
    m = len(Q)
    diag = np.diag(Q)
    scale = diag.max()
    if not scale > 0.0:
        return 0.0, np.eye(m)[0], np.eye(m, dtype=bool)[0], 0
    i0 = int(np.argmin(diag))
    tol = 64 * 2.0 ** -52 * scale
    banned = np.zeros(m, dtype=bool)
    calls = 0
    if full_start:
        S, alpha = np.ones(m, dtype=bool), np.full(m, 1.0 / m)
    else:
        S, alpha = np.eye(m, dtype=bool)[i0].copy(), np.eye(m)[i0].copy()
    for it in range(-1 if full_start else 0, 3 * m + 8):
        jb = -1
        if it >= 0:
            g = Q @ alpha
            val = alpha @ g
            free = ~(S | banned)
            if not free.any():
                break
            jb = int(np.flatnonzero(free)[np.argmin(g[free])])
            if not g[jb] < val - tol:
                break
            S[jb] = True
        for _ in range(m + 1):
            ok, beta = solve_affine(Q, scale, S)
            calls += 1
            if not ok:
                if jb < 0:      # dependent full set: the nearest vertex alone
                    S, alpha = np.eye(m, dtype=bool)[i0].copy(), np.eye(m)[i0].copy()
                else:
                    S[jb] = False
                    banned[jb] = True
                break
            neg = S & ~(beta > 0.0)
            if not neg.any():
                alpha = np.where(S, beta, 0.0)
                break
            den = alpha[neg] - beta[neg]
            r = np.where(den > 0.0, alpha[neg] / np.where(den > 0.0, den, 1.0), 0.0)
            kr = int(np.flatnonzero(neg)[np.argmin(r)])
            theta = min(1.0, float(r.min()))
            alpha = np.where(S, alpha + theta * (beta - alpha), 0.0)
            alpha[kr] = 0.0
            S[kr] = False
            if kr == jb:
                banned[jb] = True
    return float(alpha @ Q @ alpha), alpha, S, calls


def problems(X, labels, B, m, queries):
    """Gram matrices [query][bin] of the m nearest members of every bin (the query itself left out)."""
    out = []
    members = [np.flatnonzero(labels == c) for c in range(B)]
    for q in queries:
        row = []
        for c in range(B):
            ids = members[c][members[c] != q]
            d = ((X[ids] - X[q]) ** 2).sum(axis=1)
            Y = X[ids[np.argsort(d, kind="stable")[:m]]] - X[q]
            row.append(Y @ Y.T)
        out.append(row)
    return out


def wave_groups(nq, B):
    """Index lists (query, bin) of the 64 problems of a wavefront: position-major, and striped (8 positions x the bins
    c = x (mod 8) of XCD x; B = 64)."""
    plain = [[(q, c) for c in range(g, min(g + 64, B))] for q in range(nq) for g in range(0, B, 64)]
    striped = []
    for q0 in range(0, nq - 7, 8):
        for x in range(8):
            striped.append([(q, c) for q in range(q0, q0 + 8) for c in range(x, B, 8)][:64])
    return plain, striped


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, default=5)
    ap.add_argument("--queries", type=int, default=40)
    a = ap.parse_args()
    synth = load_synth()
    m = a.neighbors
    for name, mix, sigma in GENERATORS:
        X, _, true = synth.make_synthetic(a.contigs, a.dim, a.bins, S=1, seed=0, mix=mix, sigma=sigma)
        queries = np.random.default_rng(0).choice(a.contigs, a.queries, replace=False)
        G = problems(X, true, a.bins, m, queries)
        nq = len(queries)
        calls = {s: np.zeros((nq, a.bins), dtype=int) for s in (False, True)}
        sizes = np.zeros((nq, a.bins), dtype=int)
        differ = 0
        for qi in range(nq):
            for c in range(a.bins):
                v0, _, S0, calls[False][qi, c] = min_norm_point(G[qi][c], False)
                v1, _, S1, calls[True][qi, c] = min_norm_point(G[qi][c], True)
                sizes[qi, c] = int(S1.sum())
                differ += int(not np.array_equal(S0, S1))
        plain, striped = wave_groups(nq, a.bins)
        hist = np.bincount(sizes.ravel(), minlength=m + 1)[1:]
        print(f"\n{name} (mix {mix}, sigma {sigma}): N={a.contigs} D={a.dim} B={a.bins} m={m}, {nq} queries x {a.bins} bins; "
              f"final supports of the two starts differ in {differ} problems")
        print("| support size | " + " | ".join(str(k) for k in range(1, m + 1)) + " |")
        print("|---|" + "---|" * m)
        print("| share | " + " | ".join(f"{100 * h / sizes.size:.1f} %" for h in hist) + " |")
        print("| start | solves per problem | max over a wavefront's 64, one position x 64 bins (mean) | striped 8 x 8 (mean) |")
        print("|---|---|---|---|")
        for s, label in ((False, "nearest vertex"), (True, "full set")):
            wmax = [np.mean([max(calls[s][q, c] for q, c in g) for g in grp]) for grp in (plain, striped)]
            print(f"| {label} | {calls[s].mean():.2f} (max {calls[s].max()}) | {wmax[0]:.2f} | {wmax[1]:.2f} |")


if __name__ == "__main__":
    main()
