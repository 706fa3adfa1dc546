#!/usr/bin/env python3
"""Speed of the wide row-scoring calls (16 < m <= 64) against the route they replace.

Data: BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 24 and m = 64.

  wide      Context.audit_rows_wide(labels, B, m) over all rows: the tiled selection and the matrix-core hull kernel
  composed  the only route before: Context.topm_per_bin on --composed-rows rows (2048: it is far too slow for all of
            them), then Context.hull_distance_batch on the Q x B lists it returns
  tiled16   Context.audit_rows(labels, B, 16) on the same data: the scale of what a tiled call costs

All three are timed the same way in this one process after a warm-up of each: host wall-clock around calls that end in a
device synchronise; both routes are reported per row.  The split of the wide call into selection and solve is the kernel
time of chb_profile_get ("audit_wide_select" / "audit_wide_solve") from separate, profiled repeats.  The composed
route's distances are compared with the wide call's on its rows (largest difference relative to the distance).  Prints
one JSON line per m (and writes them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, nargs="+", default=[24, 64])
    ap.add_argument("--composed-rows", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B = args.contigs, args.dim, args.bins
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    Qc = min(args.composed_rows, N)
    crow = np.random.default_rng(0).choice(N, Qc, replace=False).astype(np.int64)

    _, t16 = timed(lambda: ctx.audit_rows(labels, B, 16), args.warmup, args.repeats)
    lines = []
    for m in args.neighbors:
        wide, t_wide = timed(lambda: ctx.audit_rows_wide(labels, B, m), args.warmup, args.repeats)

        def composed():
            idx, _, _ = ctx.topm_per_bin(labels, B, m, crow)
            return ctx.hull_distance_batch(np.repeat(crow, B), idx.reshape(Qc * B, m)).reshape(Qc, B)

        comp, t_comp = timed(composed, args.warmup, args.repeats)
        ctx.set_samples(X)   # (chb_topm_per_bin leaves a fit's state behind; the scoring calls use none of it)
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            ctx.audit_rows_wide(labels, B, m)
        ps, pv = ctx.profile_get("audit_wide_select"), ctx.profile_get("audit_wide_solve")
        ctx.profile_enable(False)
        fin = np.isfinite(comp)
        rel = float(np.max(np.abs(wide[1][crow][fin] - comp[fin]) / np.maximum(comp[fin], 1e-300)))
        wide_row, comp_row = t_wide["median"] / N, t_comp["median"] / Qc
        res = {
            "what": "chb_audit_rows_wide vs chb_topm_per_bin + chb_hull_distance_batch", "contigs": N, "dim": D, "bins": B,
            "neighbors": m, "warmup": args.warmup, "repeats": args.repeats, "composed_rows": Qc,
            "wide_wall_s": t_wide, "composed_wall_s": t_comp, "tiled16_wall_s": t16,
            "wide_us_per_row": wide_row * 1e6, "composed_us_per_row": comp_row * 1e6,
            "tiled16_us_per_row": t16["median"] / N * 1e6,
            "composed_over_wide_per_row": comp_row / wide_row, "wide_over_tiled16": t_wide["median"] / t16["median"],
            "wide_faster_per_row": bool(wide_row < comp_row),
            "select_kernel_s": ps["ms"] * 1e-3 / args.repeats, "solve_kernel_s": pv["ms"] * 1e-3 / args.repeats,
            "launches_per_call": ps["launches"] / args.repeats, "wide_rows": ctx.counter("recruit_wide_rows"),
            "inf_pattern_equal": bool(np.array_equal(np.isfinite(wide[1][crow]), fin)), "largest_relative_difference": rel,
        }
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
