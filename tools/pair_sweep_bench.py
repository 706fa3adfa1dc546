#!/usr/bin/env python3
"""Speed of chb_audit_pairs_multi against the calls it replaces.

Data: BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled.  Three questions:

  cohesion_narrow   every row against its OWN bin at ms = (1, 3, 5, 10, 15): one Context.audit_pairs_multi against the
                    five Context.audit_pairs calls (what five `cohesion` calls run)
  cohesion_wide     the same at ms = (5, 15, 24, 32, 64): against the five Context.audit_pairs_wide calls
  nearest_two       every row against its two nearest bins (audit_rows_nearest at k = 2, m = 15, then NearestBins.pairs)
                    at ms = (1, 3, 5, 10, 15): one Context.audit_pairs_multi against the dense Context.audit_rows_multi
                    (`neighbor_sweep`), which scores all B bins of every row

Each is timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise (medians and quartiles over the repeats), and the kernel times of chb_profile_get from
separate, profiled repeats -- the list call's "audit_pairs_multi", "audit_pairs_multi_wide_select" and
"audit_pairs_multi_wide_solve", the single calls' "audit_pairs" or "audit_pairs_wide_select" + "audit_pairs_wide_solve", the
dense sweep's "audit_multi".  Every slice of the list call is compared with its single call bit for bit (nearest_two: with
the dense sweep's entries on the first --check-rows rows).
The figure to read is multi_over_singles: the list call's time over the SUM of the calls it replaces, next to
singles_sum_spread = (q3 - q1) / median of that sum -- the run-to-run spread the ratio has to be read against.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIST_NAMES = ("audit_pairs_multi", "audit_pairs_multi_wide_select", "audit_pairs_multi_wide_solve")
SINGLE_NAMES = ("audit_pairs", "audit_pairs_wide_select", "audit_pairs_wide_solve")


def spread(t):
    q1, q3 = np.percentile(t, [25, 75])
    return {"median": float(np.median(t)), "q1": float(q1), "q3": float(q3), "min": float(np.min(t)), "max": float(np.max(t))}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def kernel_seconds(ctx, fn, names, repeats):
    """per-call kernel seconds by profile name, from `repeats` profiled calls of their own"""
    ctx.profile_reset()
    for _ in range(repeats):
        fn()
    return {k: ctx.profile_get(k)["ms"] * 1e-3 / repeats for k in names}


def compare(ctx, run_multi, run_parts, part_names, check, warmup, repeats):
    """run_multi() against the calls run_parts[key]() it replaces; check(got, outs) says whether the results agree"""
    for _ in range(warmup):
        run_multi()
        for fn in run_parts.values():
            fn()
    t_multi, t_part, equal = [], {k: [] for k in run_parts}, True
    for _ in range(repeats):   # alternating, same process
        got, dt = timed(run_multi)
        t_multi.append(dt)
        outs = {}
        for k, fn in run_parts.items():
            outs[k], dt = timed(fn)
            t_part[k].append(dt)
        equal = equal and bool(check(got, outs))
    t_sum = np.sum([t_part[k] for k in run_parts], axis=0)
    ctx.profile_enable(True)
    k_multi = kernel_seconds(ctx, run_multi, LIST_NAMES, repeats)
    k_part = {k: kernel_seconds(ctx, fn, part_names, repeats) for k, fn in run_parts.items()}
    ctx.profile_enable(False)
    k_multi_all = float(sum(k_multi.values()))
    k_sum = float(sum(sum(v.values()) for v in k_part.values()))
    s = spread(t_sum)
    return {
        "equal_bits": equal,
        "multi_wall_s": spread(t_multi),
        "singles_wall_s": {str(k): spread(v) for k, v in t_part.items()},
        "singles_sum_wall_s": s,
        "singles_sum_spread": (s["q3"] - s["q1"]) / s["median"],
        "multi_over_singles_wall": float(np.median(t_multi) / s["median"]),
        "multi_kernel_s": k_multi,
        "multi_kernel_all_s": k_multi_all,
        "singles_kernel_s": {str(k): {**v, "all": float(sum(v.values()))} for k, v in k_part.items()},
        "singles_sum_kernel_s": k_sum,
        "multi_over_singles_kernel": k_multi_all / k_sum if k_sum > 0 else None,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--narrow", type=int, nargs="+", default=[1, 3, 5, 10, 15])
    ap.add_argument("--wide", type=int, nargs="+", default=[5, 15, 24, 32, 64])
    ap.add_argument("--check-rows", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth
    from chbin_amd.clustering import NearestBins

    N, D, B = args.contigs, args.dim, args.bins
    warmup = max(args.warmup, 1)
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    rows = np.flatnonzero((labels >= 0) & (labels < B)).astype(np.int64)
    own = np.ascontiguousarray(labels[rows])
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    res = {"what": "one chb_audit_pairs_multi vs the calls it replaces", "contigs": N, "dim": D, "bins": B,
           "labelled": int(len(rows)), "warmup": warmup, "repeats": args.repeats}

    def slices_equal(ms):
        return lambda got, outs: all(same_bits(got[j], outs[m]) for j, m in enumerate(ms))

    for key, ms, single in (("cohesion_narrow", list(args.narrow), ctx.audit_pairs), ("cohesion_wide", list(args.wide), ctx.audit_pairs_wide)):
        parts = {m: (lambda m=m: single(labels, B, m, rows, own)) for m in ms}
        r = compare(ctx, lambda: ctx.audit_pairs_multi(labels, B, ms, rows, own), parts, SINGLE_NAMES, slices_equal(ms), warmup, args.repeats)
        res[key] = {"neighbors": ms, "pairs": int(len(rows)), "pair_tiles": ctx.counter("pair_tiles"), **r}

    ms = list(args.narrow)
    near = NearestBins(*ctx.audit_rows_nearest(labels, B, 15, 2))
    pos, nbins = near.pairs()
    check = np.arange(min(args.check_rows, N), dtype=np.int64)

    def dense_agrees(got, outs):
        table = ctx.audit_rows_multi(labels, B, ms, check, want_dist=True)[1]
        sel = pos < len(check)
        return same_bits(np.ascontiguousarray(got[:, sel]), np.ascontiguousarray(table[:, pos[sel], nbins[sel]]))

    r = compare(ctx, lambda: ctx.audit_pairs_multi(labels, B, ms, pos, nbins),
                {"dense": lambda: ctx.audit_rows_multi(labels, B, ms, want_dist=False)}, ("audit_multi",), dense_agrees, warmup, args.repeats)
    res["nearest_two"] = {"neighbors": ms, "pairs": int(len(pos)), "dense_problems": int(N) * int(B), **r}

    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    ctx.close()
    if not all(res[k]["equal_bits"] for k in ("cohesion_narrow", "cohesion_wide", "nearest_two")):
        sys.exit("a slice of the list call differs from the call it replaces")


if __name__ == "__main__":
    main()
