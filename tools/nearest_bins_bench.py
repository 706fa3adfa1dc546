#!/usr/bin/env python3
"""What ranking the k nearest bins on the device saves over downloading the Q x B table and sorting it on the host.

Shapes (every sample labelled, all rows scored, k = 3):
  cfg2 at m = 5 and m = 15   N = 100k, D = 136, B = 64   (BASELINE configs[2]: the table is 51 MB)
  many bins                  N = 100k, D = 32,  B = 8192, m = 3   (the documented limit: 6.5 GB, 1 GiB per chunk through
                             the pinned staging buffers and PCIe) -- the shape the call exists for

  nearest   Context.audit_rows_nearest(labels, B, m, k)
  dense     Context.audit_rows(labels, B, m, want_dist=True), then per row np.lexsort over (bin, distance) and the first k:
            what the call replaces on the parent commit

Both routes are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls
that end in a device synchronise, and the kernel times of chb_profile_get ("audit", "nearest_bins") from separate, profiled
repeats.  The two routes' results are compared bit for bit.  `nearest_bins_bytes_per_s` is the table read once, nq * B * 8
bytes per launch, over the kernel's time, beside the copy peak README.md quotes for this part (6.29 TB/s).  Prints one
JSON line per shape (and writes them to --out).

Measured (one MI355X, at the defaults, once; no ratio was fixed in advance; raw lines in profiles/r11_nearest_bins.md):
  cfg2 m = 5    nearest 0.207 s, dense 0.546 s (0.341 s the host sort); "nearest_bins" 0.069 ms of 205.5 ms of kernels, 0.74 TB/s
  cfg2 m = 15   nearest 0.252 s, dense 0.603 s (0.353 s the host sort); "nearest_bins" 0.068 ms of 249.9 ms, 0.75 TB/s
  many bins     nearest 1.197 s, dense 36.3 s (1.64 s the call with its download, 34.7 s the host sort); "nearest_bins"
                5.49 ms of 1 178 ms, 1.19 TB/s = 0.19 of the copy peak.  This is the shape the call exists for."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_PEAK_BYTES_PER_S = 6.29e12   # README.md: the measured copy peak of one MI355X

SHAPES = {
    "cfg2_m5": dict(N=100_000, D=136, B=64, m=5, warmup=1, repeats=3),
    "cfg2_m15": dict(N=100_000, D=136, B=64, m=15, warmup=1, repeats=3),
    # (819 M hull problems per call and a 6.5 GB table to sort on the host: one timed call of each route, no warm-up)
    "many_bins": dict(N=100_000, D=32, B=8192, m=3, warmup=0, repeats=1),
}


def spread(t):
    q1, q3 = np.percentile(t, [25, 75])
    return {"median": float(np.median(t)), "q1": float(q1), "q3": float(q3), "min": float(np.min(t)), "max": float(np.max(t))}


def host_rank(dist, k):
    """per row the finite entries in (distance, bin) order, the first k, padded with -1 / +inf"""
    n, B = dist.shape
    bins, out = np.full((n, k), -1, dtype=np.int64), np.full((n, k), np.inf)
    cols = np.arange(B)
    for q in range(n):
        order = np.lexsort((cols, dist[q]))[:k]
        order = order[np.isfinite(dist[q, order])]
        bins[q, :len(order)] = order
        out[q, :len(order)] = dist[q, order]
    return bins, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--contigs", type=int, default=None, help="override N of every shape")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=None, help="override the shape's warm-up calls")
    ap.add_argument("--repeats", type=int, default=None, help="override the shape's timed repeats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    ctx = _lib.default_context()
    k = args.k
    lines = []
    for name in args.shapes:
        s = SHAPES[name]
        N, D, B, m = args.contigs or s["N"], s["D"], s["B"], s["m"]
        warmup = s["warmup"] if args.warmup is None else args.warmup
        repeats = s["repeats"] if args.repeats is None else args.repeats
        X, _, labels = synth.make_synthetic(N, D, B, seed=0)
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        ctx.set_samples(X)

        def nearest():
            return ctx.audit_rows_nearest(labels, B, m, k)

        def dense():
            return host_rank(ctx.audit_rows(labels, B, m, want_dist=True)[1], k)

        def note(text):
            print(f"[{name}] {text}", file=sys.stderr, flush=True)

        for _ in range(warmup):
            nearest(), dense()
        note("timed repeats")
        t_near, t_dense, t_sort = [], [], []
        for _ in range(repeats):   # alternating, same process
            t = time.perf_counter()
            got = nearest()
            t_near.append(time.perf_counter() - t)
            note(f"nearest {t_near[-1]:.3f} s")
            t = time.perf_counter()
            table = ctx.audit_rows(labels, B, m, want_dist=True)[1]
            t1 = time.perf_counter()
            want = host_rank(table, k)
            t2 = time.perf_counter()
            t_dense.append(t2 - t)
            t_sort.append(t2 - t1)
            note(f"dense {t1 - t:.3f} s + host sort {t2 - t1:.3f} s")
            del table
        # kernel times: profiled repeats of their own
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(repeats):
            nearest()
        pa, pn = ctx.profile_get("audit"), ctx.profile_get("nearest_bins")
        note("profiled nearest done")
        ctx.profile_reset()
        for _ in range(repeats):
            ctx.audit_rows(labels, B, m, want_dist=True)
        pd = ctx.profile_get("audit")
        ctx.profile_enable(False)
        k_near = pn["ms"] * 1e-3 / repeats
        res = {
            "what": "chb_audit_rows_nearest vs chb_audit_rows(dist_out) + np.lexsort per row", "shape": name,
            "contigs": N, "dim": D, "bins": B, "neighbors": m, "k": k, "warmup": warmup, "repeats": repeats,
            "table_bytes": N * B * 8, "result_bytes": N * k * 12,
            "nearest_wall_s": spread(t_near), "dense_wall_s": spread(t_dense), "dense_host_sort_s": spread(t_sort),
            "dense_over_nearest_wall": float(np.median(t_dense) / np.median(t_near)),
            "wall_ranges_apart": bool(max(t_near) < min(t_dense)),
            "nearest_audit_kernel_s": pa["ms"] * 1e-3 / repeats, "nearest_bins_kernel_s": k_near,
            "dense_audit_kernel_s": pd["ms"] * 1e-3 / repeats,
            "nearest_bins_launches_per_call": pn["launches"] / repeats,
            "nearest_bins_work_per_call": pn["work"] / repeats,
            "nearest_bins_bytes_per_s": N * B * 8 / k_near if k_near > 0 else None,
            "copy_peak_bytes_per_s": COPY_PEAK_BYTES_PER_S,
            "nearest_bins_of_copy_peak": N * B * 8 / k_near / COPY_PEAK_BYTES_PER_S if k_near > 0 else None,
            "bitwise_equal": bool(np.array_equal(got[0], want[0]) and
                                  np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))),
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
