#!/usr/bin/env python3
"""What the witness outputs of the pair calls cost, and what they save over the composed route.

Data: BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 5 and m = 15.

  own-bin leg    every row against its own bin (clustering.cohesion's pairs): the cost of the outputs
      witness   Context.audit_pairs_witness on the N pairs (i, labels[i])
      plain     Context.audit_pairs on the same pairs
  two-bin leg    the rows of two labels against those two bins, members and weights wanted
      witness   Context.audit_pairs_witness on the 2 x (rows of the two labels) pairs
      composed  the only other route there is for ungrouped resident rows: Context.topm_per_bin over those rows (dense
                over all B bins), the two bins' lists taken out, Context.hull_distance_batch(want_alpha=True) on them

Both routes of a leg are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock
around calls that end in a device synchronise; for the own-bin leg also the kernel time of chb_profile_get
("audit_pairs", the name both routes launch under) from separate, profiled repeats of each route.  No ratio is fixed in
advance: the script prints the times and the ratios, one JSON line per m and leg (and writes them to --out).  The two
routes' distances are compared bit for bit in the own-bin leg; in the two-bin leg the index lists are compared exactly and
the distances by their largest difference (two solvers)."""
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
    from chbin_amd import _lib, synth

    N, D, B = args.contigs, args.dim, args.bins
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    every = np.arange(N, dtype=np.int64)
    a, b = args.two_bins
    two_rows = np.flatnonzero((labels == a) | (labels == b)).astype(np.int64)
    pair_rows, pair_bins = np.repeat(two_rows, 2), np.tile(np.array([a, b], dtype=np.int64), len(two_rows))

    def composed(m):
        idx, dist, _ = ctx.topm_per_bin(labels, B, m, two_rows)
        hull = np.ascontiguousarray(idx[:, [a, b]].reshape(-1, m))
        d, alpha = ctx.hull_distance_batch(pair_rows, hull, want_alpha=True)
        return d, hull, np.ascontiguousarray(dist[:, [a, b]].reshape(-1, m)), alpha

    def timed(fn, profile_name=None):
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            fn()
        p = ctx.profile_get(profile_name)
        ctx.profile_enable(False)
        return p["ms"] * 1e-3 / args.repeats, p["launches"] / args.repeats

    lines = []
    for m in args.neighbors:
        legs = {
            "own_bin": dict(witness=lambda: ctx.audit_pairs_witness(labels, B, m, every, labels),
                            other=lambda: ctx.audit_pairs(labels, B, m, every, labels),
                            other_name="chb_audit_pairs", n_pairs=N),
            "two_bins": dict(witness=lambda: ctx.audit_pairs_witness(labels, B, m, pair_rows, pair_bins),
                             other=lambda: composed(m),
                             other_name="chb_topm_per_bin + chb_hull_distance_batch", n_pairs=len(pair_rows)),
        }
        for leg, L in legs.items():
            for _ in range(args.warmup):
                got, want = L["witness"](), L["other"]()
            t_w, t_o = [], []
            for _ in range(args.repeats):   # alternating, same process
                t = time.perf_counter()
                got = L["witness"]()
                t_w.append(time.perf_counter() - t)
                t = time.perf_counter()
                want = L["other"]()
                t_o.append(time.perf_counter() - t)
            res = {
                "what": f"{leg}: chb_audit_pairs_witness vs {L['other_name']}", "leg": leg,
                "contigs": N, "dim": D, "bins": B, "neighbors": m, "warmup": args.warmup, "repeats": args.repeats,
                "pairs": L["n_pairs"], "pair_tiles": ctx.counter("pair_tiles"),
                "witness_wall_s": spread(t_w), "other_wall_s": spread(t_o),
                "witness_over_other_wall": float(np.median(t_w) / np.median(t_o)),
                "wall_ranges_apart": bool(max(t_w) < min(t_o) or max(t_o) < min(t_w)),
            }
            if leg == "own_bin":   # kernel times: profiled repeats of each route on its own (one profile name for both)
                k_w, l_w = timed(L["witness"], "audit_pairs")
                k_o, l_o = timed(L["other"], "audit_pairs")
                res.update(witness_kernel_s=k_w, other_kernel_s=k_o, witness_over_other_kernel=k_w / k_o if k_o > 0 else None,
                           witness_launches_per_call=l_w, other_launches_per_call=l_o,
                           dist_bitwise_equal=bool(np.array_equal(got[0].view(np.uint64), want.view(np.uint64))))
            else:
                fin = np.isfinite(want[0])
                res.update(lists_equal=bool(np.array_equal(got[1], want[1])),
                           list_distances_bitwise_equal=bool(np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))),
                           largest_distance_difference=float(np.abs(got[0][fin] - want[0][fin]).max()) if fin.any() else 0.0)
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
