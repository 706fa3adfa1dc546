#!/usr/bin/env python3
"""What the m <= 5 fused kernel's trim (qp_kernels.hip, "Trim") has to work on, counted on the CPU (numpy only).

For every batch of sweep 1 -- the driver's batch geometry (geom_at in chb_api.hip: a batch of at most 1.5 x the labelled
contigs) over the benchmark's generator and permutation -- a sample of positions x all bins gives the candidate count n of a
(position, bin) pair as the update-mode shortlist admits it, with exact distances in place of the fp16 bounds:

    n = min(m, base members) + batch entries at earlier positions within tau, tau = the m-th distance of the BASE members
    (more than 32 such entries: the shortlist overflows and the exact top-m of the entries stands in)

Table 1: mean n, the shares n > 7 and n > 16, and the mean n if only the union's m nearest were gathered.
Table 2: the same pairs after the trim's keep rule on the pairs with 7 < n <= 32, mirrored with the kernel's roundings
(shadow rows through float16, rho exact, the kernel's error term E on T = ||Gs[j] - Gs[p]||^2): drop p only if
sqrt(max(T - E, 0)) - rho_j - rho_p > tau_u (1 + 1e-6), tau_u the m-th smallest sqrt(T + E) + rho_j + rho_p.

usage: tools/fused_trim_probe.py [--contigs N] [--dim D] [--bins B] [--neighbors m] [--mix x] [--sigma s] [--sample k]
"""
import argparse
import importlib.util
import os

import numpy as np

C_NARROW = 7      # CHB_FUSED_C: widest shortlist of the one-sweep form
WIDE = 16         # kFusedWide
TRIM_MAX = 32     # kTrimMax
CAP_U = 32        # kCandCapU
SLACK = 1e-6      # kTrimSlack
GAMMA = 2.5e-5    # kTrimGamma


def load_synth():
    """ch-bin_amd/synth.py without importing the package (which loads the GPU library)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("chb_synth", os.path.join(root, "ch-bin_amd", "synth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def shadow_scale(X):
    """(mu_g, S) as samples_finish picks them for rows of one slice: S = 2^(10 - e), max |x - mu_g| < 2^e."""
    mu = X.mean(axis=0)
    R = float(np.float32(np.abs(X - mu).max()))
    if not (R > 0.0 and np.isfinite(R)):
        return mu, 1.0
    return mu, float(np.ldexp(1.0, 10 - int(np.frexp(R)[1])))


def shadows(X, mu, S):
    """Gs (the float16 rows as float64) and rho of every sample: global_shadow_kernel."""
    Z = (X - mu) * S
    G = np.clip(Z.astype(np.float32), -65504.0, 65504.0).astype(np.float16).astype(np.float64)
    return G, np.sqrt(((G - Z) ** 2).sum(axis=1))


def trim_keep(gj, rho_j, G, rho, m):
    """The keep rule on one pair: gj / rho_j = the query's shadow row and radius, G / rho = the candidates'.  A non-finite
    bound keeps everything; a comparison with NaN keeps the candidate."""
    D = len(gj)
    Nj, Np = (gj ** 2).sum(), (G ** 2).sum(axis=1)
    T = ((gj[None, :] - G) ** 2).sum(axis=1)
    E = (2 * GAMMA * np.sqrt(Nj * Np) + 2.0 ** -23 * (Nj + Np) + 2.0 ** -13 * np.sqrt(D) * (np.sqrt(Nj) + np.sqrt(Np))
         + 2.0 ** -27 * D)
    with np.errstate(invalid="ignore"):
        lo = np.sqrt(np.maximum(T - E, 0.0)) - rho_j - rho
        hi = np.sqrt(T + E) + rho_j + rho
    if not np.all(np.isfinite(hi)) or len(hi) < m:
        return np.ones(len(hi), dtype=bool)
    tau = np.sort(hi)[m - 1]
    return ~(lo > tau * (1.0 + SLACK))


def batches_of_sweep1(n_seeded, n_move, kmax=8192):
    """(t0, K) of sweep 1's batches: geom_at."""
    t, out = 0, []
    while t < n_move:
        K = min(kmax, n_move - t)
        members = (n_seeded + t) * 3 // 2
        if members < K:
            K = max(min(64, n_move - t), members)
        out.append((t, min(K, kmax)))
        t += out[-1][1]
    return out


def pair_candidates(X, lab, base, entries, j, B, m):
    """Candidate ids of the pairs (j, every bin): base = labelled samples outside the batch, entries = the batch entries
    eligible for j, both index arrays; lab = the labels in force.  Returns a list of B index arrays, base candidates first."""
    db = np.sqrt(((X[base] - X[j]) ** 2).sum(axis=1))
    du = np.sqrt(((X[entries] - X[j]) ** 2).sum(axis=1)) if len(entries) else np.zeros(0)
    out = []
    for c in range(B):
        ib = np.flatnonzero(lab[base] == c)
        ob = ib[np.argsort(db[ib], kind="stable")][:m]
        tau = db[ob[-1]] if len(ob) == m else np.inf
        iu = np.flatnonzero(lab[entries] == c) if len(entries) else np.zeros(0, dtype=np.int64)
        iu = iu[du[iu] <= tau]
        if len(iu) > CAP_U:   # overflow: the exact top-m of the entries
            iu = iu[np.argsort(du[iu], kind="stable")][:m]
        out.append(np.concatenate([base[ob], entries[iu]]).astype(np.int64))
    return out


def probe(X, initial, perm, lab_after, B, m, sample, rng, kmax=8192):
    """Rows (t0, K, labelled, mean n, share n > 7, share n > 16, mean min(n, m), mean n', share n' > 7, max n', mean rho)."""
    mu, S = shadow_scale(X)
    G, rho = shadows(X, mu, S)
    lab = initial.copy()
    rows = []
    for t0, K in batches_of_sweep1(int((initial >= 0).sum()), len(perm), kmax):
        base = np.flatnonzero(lab >= 0)
        batch = perm[t0:t0 + K]
        labb = lab.copy()
        labb[batch] = lab_after[batch]
        ns, nt = [], []
        for p in np.sort(rng.choice(K, min(sample, K), replace=False)):
            j = batch[p]
            for ids in pair_candidates(X, labb, base, batch[:p], j, B, m):
                n = len(ids)
                ns.append(n)
                if C_NARROW < n <= TRIM_MAX:
                    n = int(trim_keep(G[j], rho[j], G[ids], rho[ids], m).sum())
                nt.append(n)
        ns, nt = np.array(ns), np.array(nt)
        rows.append((t0, K, len(base), ns.mean(), (ns > C_NARROW).mean(), (ns > WIDE).mean(), np.minimum(ns, m).mean(),
                     nt.mean(), (nt > C_NARROW).mean(), nt.max(), rho.mean()))
        lab[batch] = lab_after[batch]
    return rows, S


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, default=5)
    ap.add_argument("--mix", type=float, default=0.0)
    ap.add_argument("--sigma", type=float, default=1.5e-3)
    ap.add_argument("--sample", type=int, default=50, help="positions sampled per batch")
    a = ap.parse_args()
    synth = load_synth()
    X, initial, true = synth.make_synthetic(a.contigs, a.dim, a.bins, seed=0, mix=a.mix, sigma=a.sigma)
    perm = synth.draw_permutations(initial, 1, seed=0)[0]
    # (the labels sweep 1 hands out: the generator's bins stand in for them -- numpy only)
    rows, S = probe(X, initial, perm, true, a.bins, a.neighbors, a.sample, np.random.default_rng(0))
    print(f"N={a.contigs} D={a.dim} B={a.bins} m={a.neighbors} mix={a.mix} sigma={a.sigma}: S = 2^{int(np.log2(S))}, "
          f"mean rho {rows[0][-1]:.3g} (shadow units)")
    print("| batch (positions, labelled before it) | mean n | n > 7 | n > 16 | mean min(n, m) | trimmed: mean n | n > 7 | max n |")
    print("|---|---|---|---|---|---|---|---|")
    for i, (t0, K, nl, mn, w7, w16, mm, tn, t7, tmax, _) in enumerate(rows):
        print(f"| {i} ({K:,}; {nl:,}) | {mn:.2f} | {100 * w7:.1f} % | {100 * w16:.1f} % | {mm:.2f} | {tn:.2f} | "
              f"{100 * t7:.3f} % | {tmax} |")


if __name__ == "__main__":
    main()
