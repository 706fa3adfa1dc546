#!/usr/bin/env python3
"""Speed of chb_audit_rows_multi against the single chb_audit_rows calls it replaces.

Question: the leave-one-out hull distance of EVERY resident row to every bin of a frozen labelling at every m of a list
(default: the data of BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 1, 3, 5, 10, 15).

  multi    one Context.audit_rows_multi(labels, B, ms) on a context that holds X
  singles  on the same context: Context.audit_rows(labels, B, m) for every m of the list, one after the other

Both are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise, and the kernel time of chb_profile_get("audit_multi") / ("audit") from separate, profiled
repeats.  Every slice of the list call is compared with its single call for equality.  The figure to read is
multi_over_singles: the list call's time over the SUM of the single calls' times (below 1: the list call is faster), on
the wall clock and on the kernels alone; multi_over_largest_single says how much the list costs on top of the one call at
max(ms) whose selection stream it shares.  Prints one JSON line (and writes it to --out)."""
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
    ap.add_argument("--neighbors", type=int, nargs="+", default=[1, 3, 5, 10, 15])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B, ms = args.contigs, args.dim, args.bins, list(args.neighbors)
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    members = int(np.count_nonzero((labels >= 0) & (labels < B)))
    ctx = _lib.Context(0)
    ctx.set_samples(X)

    def run_multi():
        return ctx.audit_rows_multi(labels, B, ms)

    def run_single(m):
        return ctx.audit_rows(labels, B, m)

    for _ in range(max(args.warmup, 1)):
        got = run_multi()
        for m in ms:
            run_single(m)
    t_multi, t_single = [], {m: [] for m in ms}
    equal = True
    for _ in range(args.repeats):   # alternating, same process
        t = time.perf_counter()
        got = run_multi()
        t_multi.append(time.perf_counter() - t)
        for j, m in enumerate(ms):
            t = time.perf_counter()
            one = run_single(m)
            t_single[m].append(time.perf_counter() - t)
            equal = equal and all(np.array_equal(a[j], b) for a, b in zip(got, one))
    t_sum = np.sum([t_single[m] for m in ms], axis=0)
    # kernel time: profiled repeats of their own, one profile per call kind
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.repeats):
        run_multi()
    pm = ctx.profile_get("audit_multi")
    kernel_single = {}
    for m in ms:
        ctx.profile_reset()
        for _ in range(args.repeats):
            run_single(m)
        kernel_single[m] = ctx.profile_get("audit")["ms"] * 1e-3 / args.repeats
    ctx.profile_enable(False)
    kernel_multi = pm["ms"] * 1e-3 / args.repeats
    kernel_sum = float(sum(kernel_single.values()))
    m_max = max(ms)

    res = {
        "what": "one chb_audit_rows_multi over all rows vs one chb_audit_rows per m",
        "contigs": N, "dim": D, "bins": B, "neighbors": ms, "labelled": members,
        "warmup": max(args.warmup, 1), "repeats": args.repeats,
        "rows_per_launch": ctx.counter("recruit_multi_rows"),
        "every_slice_equal": bool(equal),
        "multi_wall_s": spread(t_multi),
        "singles_wall_s": {str(m): spread(t_single[m]) for m in ms},
        "singles_sum_wall_s": spread(t_sum),
        "multi_over_singles_wall": float(np.median(t_multi) / np.median(t_sum)),
        "multi_over_largest_single_wall": float(np.median(t_multi) / np.median(t_single[m_max])),
        "multi_kernel_s": kernel_multi,
        "multi_kernel_launches_per_call": pm["launches"] / args.repeats,
        "multi_triples_per_call": pm["work"] / args.repeats,
        "singles_kernel_s": {str(m): kernel_single[m] for m in ms},
        "singles_sum_kernel_s": kernel_sum,
        "multi_over_singles_kernel": kernel_multi / kernel_sum if kernel_sum > 0 else None,
        "multi_over_largest_single_kernel": kernel_multi / kernel_single[m_max] if kernel_single[m_max] > 0 else None,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    ctx.close()
    if not equal:
        sys.exit("a slice of the list call differs from its single call")


if __name__ == "__main__":
    main()
