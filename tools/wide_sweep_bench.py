#!/usr/bin/env python3
"""Speed of chb_audit_rows_multi_wide against the single chb_audit_rows_wide calls it replaces.

Question: the leave-one-out hull distance of EVERY resident row to every bin of a frozen labelling at every m of a list
with entries above 16 (default: the data of BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at
m = 5, 15, 24, 32, 64).

  multi    one Context.audit_rows_multi_wide(labels, B, ms) on a context that holds X
  singles  on the same context: Context.audit_rows_wide(labels, B, m) for every m of the list, one after the other

Both are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise, and the kernel times of chb_profile_get from separate, profiled repeats -- the list call's
"audit_multi" (its entries up to 16), "audit_multi_wide_select" and "audit_multi_wide_solve", the single calls' "audit" or
"audit_wide_select" + "audit_wide_solve".  Every slice of the list call is compared with its single call bit for bit.
The figure to read is multi_over_singles: the list call's time over the SUM of the single calls' times.  The list call does
a strict subset of their device work (one tiled selection in place of one per entry up to 16, one wide selection in place
of one per entry above; the hull solves are the single calls'), so anything at or above 1 is a finding.  multi_over_largest_single says what the list costs on top of the one call at max(ms)
whose selection stream it shares.  Prints one JSON line (and writes it to --out)."""
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


def same_bits(a, b):
    if a.dtype.kind == "f":
        return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    return np.array_equal(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, nargs="+", default=[5, 15, 24, 32, 64])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B, ms = args.contigs, args.dim, args.bins, list(args.neighbors)
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    members = int(np.count_nonzero((labels >= 0) & (labels < B)))
    ctx = _lib.Context(0)
    ctx.set_samples(X)

    def run_multi():
        return ctx.audit_rows_multi_wide(labels, B, ms)

    def run_single(m):
        return ctx.audit_rows_wide(labels, B, m)

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
            equal = equal and all(same_bits(a[j], b) for a, b in zip(got, one))
    t_sum = np.sum([t_single[m] for m in ms], axis=0)
    # kernel time: profiled repeats of their own, one profile per call kind
    multi_names = ("audit_multi", "audit_multi_wide_select", "audit_multi_wide_solve")
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.repeats):
        run_multi()
    wide_rows = ctx.counter("recruit_wide_rows")
    pm = {k: ctx.profile_get(k) for k in multi_names}
    kernel_single = {}
    for m in ms:
        ctx.profile_reset()
        for _ in range(args.repeats):
            run_single(m)
        part = {k: ctx.profile_get(k)["ms"] * 1e-3 / args.repeats for k in ("audit", "audit_wide_select", "audit_wide_solve")}
        kernel_single[m] = {"select": part["audit_wide_select"], "solve": part["audit_wide_solve"], "tiled": part["audit"],
                            "all": sum(part.values())}
    ctx.profile_enable(False)
    kernel_multi = {k: pm[k]["ms"] * 1e-3 / args.repeats for k in multi_names}
    kernel_multi_all = float(sum(kernel_multi.values()))
    kernel_sum = float(sum(v["all"] for v in kernel_single.values()))
    m_max = max(ms)

    res = {
        "what": "one chb_audit_rows_multi_wide over all rows vs one chb_audit_rows_wide per m",
        "contigs": N, "dim": D, "bins": B, "neighbors": ms, "labelled": members,
        "warmup": max(args.warmup, 1), "repeats": args.repeats,
        "rows_per_launch": wide_rows,
        "every_slice_equal": bool(equal),
        "multi_wall_s": spread(t_multi),
        "singles_wall_s": {str(m): spread(t_single[m]) for m in ms},
        "singles_sum_wall_s": spread(t_sum),
        "multi_over_singles_wall": float(np.median(t_multi) / np.median(t_sum)),
        "multi_over_largest_single_wall": float(np.median(t_multi) / np.median(t_single[m_max])),
        "multi_faster_than_singles": bool(np.median(t_multi) < np.median(t_sum)),
        "multi_kernel_s": kernel_multi,
        "multi_kernel_all_s": kernel_multi_all,
        "multi_select_launches_per_call": pm["audit_multi_wide_select"]["launches"] / args.repeats,
        "multi_solve_triples_per_call": pm["audit_multi_wide_solve"]["work"] / args.repeats,
        "singles_kernel_s": {str(m): kernel_single[m] for m in ms},
        "singles_sum_kernel_s": kernel_sum,
        "multi_over_singles_kernel": kernel_multi_all / kernel_sum if kernel_sum > 0 else None,
        "multi_over_largest_single_kernel": kernel_multi_all / kernel_single[m_max]["all"] if kernel_single[m_max]["all"] > 0 else None,
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
