#!/usr/bin/env python3
"""Speed of the wide report calls (16 < m <= 64) against the routes they replace.

Data: BASELINE configs[2] -- N = 100k, D = 136, B = 64, every sample labelled -- at m = 24 and m = 64.

  nearest   Context.audit_rows_nearest_wide(labels, B, m, k) over all rows
            against Context.audit_rows_wide(want_dist=True) and np.lexsort over (row, distance, bin) on the host
  report    Context.bin_report_wide(labels, B, m)
            against Context.audit_rows_wide(want_dist=True) and the numpy reduction of the N x B table per own label
  witness   Context.audit_pairs_witness_wide over every row's own bin (N pairs)
            against Context.audit_pairs_wide(want_idx=True) and Context.hull_distance_batch on the lists it returns
            (which gives the distances only: there was no route to the weights)

Every route is timed the same way in this one process after a warm-up of each: host wall-clock around calls that end in
a device synchronise.  The outputs of the two routes are compared (bins and counts exactly; distances by their bits
where both come from the wide kernels, else by the largest relative difference).  Prints one JSON line per m (and writes
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


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}


def rank_on_host(dist, k):
    """the k nearest bins per row of a [Q, B] table by (distance, bin), -1 / +inf where the row has fewer finite entries"""
    Q, B = dist.shape
    order = np.lexsort((np.tile(np.arange(B), Q), dist.ravel(), np.repeat(np.arange(Q), B))).reshape(Q, B)[:, :k] % B
    nd = np.take_along_axis(dist, order, axis=1)
    return np.where(np.isfinite(nd), order, -1), nd


def reduce_on_host(labels, B, bins, dist):
    conf = np.zeros((B, B), dtype=np.int64)
    unplaced = np.zeros(B, dtype=np.int64)
    dcnt = np.zeros((B, B), dtype=np.int64)
    dmin = np.full((B, B), np.inf)
    dsum = np.zeros((B, B))
    for a in range(B):
        sel = labels == a
        bn, d = bins[sel], dist[sel]
        conf[a] = np.bincount(bn[bn >= 0], minlength=B)
        unplaced[a] = np.count_nonzero(bn < 0)
        fin = np.isfinite(d)
        dcnt[a] = fin.sum(axis=0)
        dmin[a] = np.where(fin, d, np.inf).min(axis=0, initial=np.inf)
        dsum[a] = np.where(fin, d, 0.0).sum(axis=0)
    return conf, unplaced, dcnt, dmin, dsum


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, nargs="+", default=[24, 64])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B, k = args.contigs, args.dim, args.bins, args.k
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    rows = np.arange(N, dtype=np.int64)
    ctx = _lib.Context(0)
    ctx.set_samples(X)
    lines = []
    for m in args.neighbors:
        near, t_near = timed(lambda: ctx.audit_rows_nearest_wide(labels, B, m, k), args.warmup, args.repeats)

        def near_host():
            return rank_on_host(ctx.audit_rows_wide(labels, B, m)[1], k)

        near_h, t_near_h = timed(near_host, args.warmup, args.repeats)
        rep, t_rep = timed(lambda: ctx.bin_report_wide(labels, B, m), args.warmup, args.repeats)

        def rep_host():
            bins, dist, _, _ = ctx.audit_rows_wide(labels, B, m)
            return reduce_on_host(labels, B, bins, dist)

        rep_h, t_rep_h = timed(rep_host, args.warmup, args.repeats)
        wit, t_wit = timed(lambda: ctx.audit_pairs_witness_wide(labels, B, m, rows, labels), args.warmup, args.repeats)

        def wit_composed():
            dist, idx = ctx.audit_pairs_wide(labels, B, m, rows, labels, want_idx=True)
            return dist, idx, ctx.hull_distance_batch(rows, idx)

        wit_c, t_wit_c = timed(wit_composed, args.warmup, args.repeats)
        _, t_pairs = timed(lambda: ctx.audit_pairs_wide(labels, B, m, rows, labels), args.warmup, args.repeats)
        fin = np.isfinite(wit_c[2])
        res = {
            "what": "chb_*_wide report calls vs chb_audit_rows_wide / chb_audit_pairs_wide + host or composed routes",
            "contigs": N, "dim": D, "bins": B, "neighbors": m, "k": k, "warmup": args.warmup, "repeats": args.repeats,
            "nearest_wall_s": t_near, "nearest_host_wall_s": t_near_h,
            "nearest_host_over_device": t_near_h["median"] / t_near["median"],
            "nearest_equal": bool(np.array_equal(near[0], near_h[0]) and np.array_equal(bits(near[1]), bits(near_h[1]))),
            "report_wall_s": t_rep, "report_host_wall_s": t_rep_h,
            "report_host_over_device": t_rep_h["median"] / t_rep["median"],
            "report_equal": bool(all(np.array_equal(a, b) for a, b in zip(rep[:4], rep_h[:4]))),
            "report_dsum_largest_relative_difference":
                float(np.max(np.abs(rep[4] - rep_h[4]) / np.maximum(np.abs(rep_h[4]), 1e-300))),
            "witness_wall_s": t_wit, "witness_composed_wall_s": t_wit_c, "pairs_wide_wall_s": t_pairs,
            "witness_composed_over_device": t_wit_c["median"] / t_wit["median"],
            "witness_over_plain_pairs": t_wit["median"] / t_pairs["median"],
            "witness_dist_equal": bool(np.array_equal(bits(wit[0]), bits(wit_c[0])) and np.array_equal(wit[1], wit_c[1])),
            "witness_composed_largest_relative_difference":
                float(np.max(np.abs(wit[0][fin] - wit_c[2][fin]) / np.maximum(wit_c[2][fin], 1e-300))),
            "wide_rows": ctx.counter("recruit_wide_rows"),
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
