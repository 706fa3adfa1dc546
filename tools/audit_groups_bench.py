#!/usr/bin/env python3
"""Cost of the leave-group-out audit (chb_audit_rows_grouped) next to the leave-one-out audit (chb_audit_rows) and next to
the route it replaces.

Question: the hull distance of EVERY resident row to every bin of a frozen labelling with all pieces of the row's parent
contig withheld (default: N = 100k, D = 136, B = 64, every sample labelled, --sub = 4 pieces per parent assigned as in
tools/cli_config4.py, so that siblings are not neighbours in the table; m = 5 and m = 15).

  grouped     Context.audit_rows_grouped(labels, groups, B, m) over all rows
  ungrouped   Context.audit_rows(labels, B, m) over all rows on the same context and data: the yardstick.  Its kernel's
              instruction stream does not change with the grouped instantiations, so its time is the time of
              the library before them
  per parent  what the grouped call replaces: one chb_audit_rows call per parent for the parent's rows on the labels with
              those rows set to -1.  Timed on a sample of --parents parents and extrapolated linearly to all of them (the
              cost is linear in the number of calls: each builds and uploads its own CSR over the labels)

grouped and ungrouped alternate in this one process after a warm-up of each: host wall-clock around calls that end in a
device synchronise, and the kernel time of chb_profile_get("audit") from separate, profiled repeats.  The sampled
parents' rows of the grouped table are compared bit for bit with the per-parent route.  One JSON line per m (--out)."""
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
    ap.add_argument("--sub", type=int, default=4, help="pieces per parent contig")
    ap.add_argument("--parents", type=int, default=200, help="parents timed on the per-parent route")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B = args.contigs, args.dim, args.bins
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    order = np.random.default_rng(1).permutation(N)   # pieces of a parent are not neighbours in the table
    groups = np.empty(N, dtype=np.int64)
    groups[order] = np.arange(N) // args.sub
    n_par = int(groups.max()) + 1
    by_parent = np.argsort(groups, kind="stable")
    starts = np.searchsorted(groups[by_parent], np.arange(n_par + 1))
    sample = np.random.default_rng(2).choice(n_par, min(args.parents, n_par), replace=False)
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    lines = []
    for m in args.neighbors:
        def run_grouped():
            return ctx.audit_rows_grouped(labels, groups, B, m)

        def run_plain():
            return ctx.audit_rows(labels, B, m)

        def run_per_parent():
            out = {}
            for g in sample:
                rows = by_parent[starts[g]:starts[g + 1]].astype(np.int64)
                lab = labels.copy()
                lab[rows] = -1
                out[int(g)] = (rows, ctx.audit_rows(lab, B, m, rows))
            return out

        for _ in range(args.warmup):
            run_grouped()
            run_plain()
        t_grouped, t_plain = [], []
        for _ in range(args.repeats):   # alternating, same process
            t = time.perf_counter()
            got = run_grouped()
            t_grouped.append(time.perf_counter() - t)
            t = time.perf_counter()
            plain = run_plain()
            t_plain.append(time.perf_counter() - t)
        t = time.perf_counter()
        route = run_per_parent()
        t_route = time.perf_counter() - t
        # kernel time: profiled repeats of their own
        kernel = {}
        ctx.profile_enable(True)
        for name, fn in (("grouped", run_grouped), ("ungrouped", run_plain)):
            ctx.profile_reset()
            for _ in range(args.repeats):
                fn()
            kernel[name] = ctx.profile_get("audit")
        ctx.profile_enable(False)
        k_grouped = kernel["grouped"]["ms"] * 1e-3 / args.repeats
        k_plain = kernel["ungrouped"]["ms"] * 1e-3 / args.repeats

        same = all(np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                  b[rows].view(np.uint64) if b.dtype == np.float64 else b[rows])
                   for rows, res in route.values() for a, b in zip(res, got))
        res = {
            "what": "chb_audit_rows_grouped over all rows vs chb_audit_rows, and vs one chb_audit_rows call per parent",
            "contigs": N, "dim": D, "bins": B, "neighbors": m, "pieces_per_parent": args.sub, "parents": n_par,
            "warmup": args.warmup, "repeats": args.repeats,
            "grouped_wall_s": spread(t_grouped),
            "ungrouped_wall_s": spread(t_plain),
            "grouped_over_ungrouped_wall": float(np.median(t_grouped) / np.median(t_plain)),
            "grouped_kernel_s": k_grouped,
            "ungrouped_kernel_s": k_plain,
            "grouped_over_ungrouped_kernel": k_grouped / k_plain if k_plain > 0 else None,
            "launches_per_call": [kernel["grouped"]["launches"] / args.repeats, kernel["ungrouped"]["launches"] / args.repeats],
            "per_parent_sample": len(sample),
            "per_parent_sample_s": t_route,
            "per_parent_all_s_extrapolated": t_route / len(sample) * n_par,
            "per_parent_over_grouped": t_route / len(sample) * n_par / float(np.median(t_grouped)),
            "sample_rows_same_bits_as_per_parent_route": bool(same),
            "rows_whose_distances_differ_from_leave_one_out": int(np.count_nonzero((got[1] != plain[1]).any(axis=1))),
            "rows_whose_bin_is_not_their_label": [int(np.count_nonzero(got[0] != labels)), int(np.count_nonzero(plain[0] != labels))],
        }
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
