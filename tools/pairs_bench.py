#!/usr/bin/env python3
"""Speed of the pair calls against the dense route of the same library for two sparse questions.

Data: BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 5 and m = 15.

  own-bin leg    how well does every contig sit in its own bin?
      pairs   clustering.cohesion over all rows (chb_audit_pairs on the N pairs (i, labels[i]))
      dense   Context.audit_rows(labels, B, m) with dist_out, then each row's own entry
  two-bin leg    the rows of two labels against those two bins (what BinReport.confused_pairs leads to)
      pairs   Context.audit_pairs on the 2 x (rows of the two labels) pairs
      dense   Context.audit_rows(labels, B, m, rows=those rows), then the two columns

Both routes of a leg are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock
around calls that end in a device synchronise, and the kernel time of chb_profile_get ("audit_pairs" / "audit") from
separate, profiled repeats.  The results of the two routes are compared bit for bit.  By the members streamed the pair
route of the own-bin leg needs 1 / B of the dense kernel's selection work (`estimate`), that of the two-bin leg 2 / B;
`achieved_of_estimate` is estimate over the measured kernel-time ratio.  Prints one JSON line per m and leg (and writes
them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(t):
    q1, q3 = np.percentile(t, [25, 75])
    return {"median": float(np.median(t)), "q1": float(q1), "q3": float(q3), "min": float(np.min(t)), "max": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, nargs="+", default=[5, 15])
    ap.add_argument("--two-bins", type=int, nargs=2, default=[7, 12])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, clustering, synth

    N, D, B = args.contigs, args.dim, args.bins
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    ctx = _lib.default_context()   # (clustering.cohesion's context)
    ctx.set_samples(X)
    every = np.arange(N, dtype=np.int64)
    a, b = args.two_bins
    two_rows = np.flatnonzero((labels == a) | (labels == b)).astype(np.int64)
    pair_rows, pair_bins = np.repeat(two_rows, 2), np.tile(np.array([a, b], dtype=np.int64), len(two_rows))

    lines = []
    for m in args.neighbors:
        legs = {
            "own_bin": dict(
                pairs=lambda: clustering.cohesion(X, labels, B, num_neighbors=m),
                dense=lambda: ctx.audit_rows(labels, B, m)[1][every, labels],
                n_pairs=N, dense_pairs=N * B, estimate=1.0 / B),
            "two_bins": dict(
                pairs=lambda: ctx.audit_pairs(labels, B, m, pair_rows, pair_bins),
                dense=lambda: ctx.audit_rows(labels, B, m, two_rows)[1][:, [a, b]].reshape(-1),
                n_pairs=len(pair_rows), dense_pairs=len(two_rows) * B, estimate=2.0 / B),
        }
        for leg, L in legs.items():
            for _ in range(args.warmup):
                got, want = L["pairs"](), L["dense"]()
            t_pairs, t_dense = [], []
            for _ in range(args.repeats):   # alternating, same process
                t = time.perf_counter()
                got = L["pairs"]()
                t_pairs.append(time.perf_counter() - t)
                t = time.perf_counter()
                want = L["dense"]()
                t_dense.append(time.perf_counter() - t)
            tiles = ctx.counter("pair_tiles")
            # kernel times: profiled repeats of their own
            ctx.profile_enable(True)
            ctx.profile_reset()
            for _ in range(args.repeats):
                L["pairs"]()
                L["dense"]()
            pp, pd = ctx.profile_get("audit_pairs"), ctx.profile_get("audit")
            ctx.profile_enable(False)
            k_pairs, k_dense = pp["ms"] * 1e-3 / args.repeats, pd["ms"] * 1e-3 / args.repeats
            ratio = k_pairs / k_dense if k_dense > 0 else None
            res = {
                "what": f"{leg}: chb_audit_pairs vs chb_audit_rows + gather", "leg": leg,
                "contigs": N, "dim": D, "bins": B, "neighbors": m, "warmup": args.warmup, "repeats": args.repeats,
                "pairs": L["n_pairs"], "dense_grid": L["dense_pairs"], "pair_tiles": tiles,
                "pairs_wall_s": spread(t_pairs), "dense_wall_s": spread(t_dense),
                "dense_over_pairs_wall": float(np.median(t_dense) / np.median(t_pairs)),
                "wall_ranges_apart": bool(max(t_pairs) < min(t_dense)),
                "pairs_kernel_s": k_pairs, "dense_kernel_s": k_dense,
                "pairs_launches_per_call": pp["launches"] / args.repeats,
                "dense_launches_per_call": pd["launches"] / args.repeats,
                "pairs_work_per_call": pp["work"] / args.repeats,
                "kernel_ratio": ratio, "estimate": L["estimate"],
                "achieved_of_estimate": L["estimate"] / ratio if ratio else None,
                "bitwise_equal": bool(np.array_equal(np.asarray(got).view(np.uint64),
                                                     np.ascontiguousarray(want).view(np.uint64))),
            }
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
