#!/usr/bin/env python3
"""Speed of chb_audit_rows against what the library could do for the same question before it existed.

Question: the leave-one-out hull distance of EVERY resident row to every bin of a frozen labelling (default: the data of
BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 5 and m = 15).

  new       Context.audit_rows(labels, B, m) on a context that holds X
  baseline  on the same context: topm_per_bin for the same rows, then hull_distance_batch on the lists it returns, in
            slices of --baseline-slice rows (the lists of all rows at once are Q x B x m int64 indices plus as many doubles
            on the host: 1.5 GB at m = 15)

Both are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise, and for the new call the kernel time of chb_profile_get("audit") from separate, profiled
repeats.  The two results are compared entry by entry.  Prints one JSON line per m (and writes them to --out).

Roofline figure of the new kernel, as in tools/recruit_bench.py: the selection needs Q x (labelled samples) x D subtract /
multiply / add triples in fp64 VALU (three instructions, nothing fuses under cdist's rounding) against 39.3e12 fp64
lane-instructions per second."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_VALU_LANE_OPS = 78.6e12 / 2.0   # fp64 vector instructions x lanes per second


def spread(t):
    q1, q3 = np.percentile(t, [25, 75])
    return {"median": float(np.median(t)), "q1": float(q1), "q3": float(q3), "min": float(np.min(t)), "max": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, nargs="+", default=[5, 15])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-slice", type=int, default=25_000)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B = args.contigs, args.dim, args.bins
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    members = int(np.count_nonzero((labels >= 0) & (labels < B)))
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    rows = np.arange(N, dtype=np.int64)
    lines = []
    for m in args.neighbors:
        def run_new():
            return ctx.audit_rows(labels, B, m)

        def run_base():
            out = np.empty((N, B))
            for r0 in range(0, N, args.baseline_slice):
                q = rows[r0:r0 + args.baseline_slice]
                idx, _, _ = ctx.topm_per_bin(labels, B, m, q)
                out[r0:r0 + len(q)] = ctx.hull_distance_batch(np.repeat(q, B), idx.reshape(len(q) * B, m)).reshape(len(q), B)
            return out

        want = None
        for _ in range(args.warmup):
            got = run_new()
            want = None if args.no_baseline else run_base()
        t_new, t_base = [], []
        for _ in range(args.repeats):   # alternating, same process
            t = time.perf_counter()
            got = run_new()
            t_new.append(time.perf_counter() - t)
            if not args.no_baseline:
                t = time.perf_counter()
                want = run_base()
                t_base.append(time.perf_counter() - t)
        # kernel time: profiled repeats of their own
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            run_new()
        prof = ctx.profile_get("audit")
        ctx.profile_enable(False)
        kernel_s = prof["ms"] * 1e-3 / args.repeats

        triples = float(N) * members * D
        res = {
            "what": "chb_audit_rows over all rows vs topm_per_bin + hull_distance_batch",
            "contigs": N, "dim": D, "bins": B, "neighbors": m, "labelled": members,
            "warmup": args.warmup, "repeats": args.repeats,
            "new_wall_s": spread(t_new),
            "new_kernel_s": kernel_s,
            "new_kernel_launches_per_call": prof["launches"] / args.repeats,
            "new_pairs_per_call": prof["work"] / args.repeats,
            "selection_triples": triples,
            "triples_per_s": triples / kernel_s if kernel_s > 0 else None,
            "fp64_valu_fraction": 3.0 * triples / kernel_s / FP64_VALU_LANE_OPS if kernel_s > 0 else None,
        }
        if want is not None:
            fin = np.isfinite(want)
            res.update({
                "baseline_wall_s": spread(t_base),
                "baseline_slice": args.baseline_slice,
                "baseline_over_new_wall": float(np.median(t_base) / np.median(t_new)),
                "same_inf_pattern": bool(np.array_equal(fin, np.isfinite(got[1]))),
                "max_abs_difference": float(np.abs(got[1][fin] - want[fin]).max()) if fin.any() else 0.0,
                "same_bins": bool(np.array_equal(got[0], np.argmin(want, axis=1))),
                "rows_whose_bin_is_not_their_label": int(np.count_nonzero(got[0] != labels)),
            })
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
