#!/usr/bin/env python3
"""Speed of chb_bin_report against what the library could do for the same question before it existed.

Question: per (own bin, bin) pair of a labelling, how many rows of the own bin would choose the other one now, and count /
minimum / sum of their leave-one-out hull distances to it (default: the data of BASELINE configs[2] -- N = 100k, D = 136,
B = 64, every sample labelled -- at m = 5).

  new       Context.bin_report(labels, B, m) on a context that holds X: only the five tables cross the host boundary
  baseline  on the same context: Context.audit_rows(labels, B, m) with dist_out -- the whole Q x B table comes down through
            the pinned staging halves -- and the same reduction by the rows' own labels in numpy

Both are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise.  The kernel split ("audit" = selection + hull kernel and row reduction, "bin_report" = the
fold into the tables) comes from chb_profile_get in separate, profiled repeats of the new call.  The two results are
compared: counts and minima exactly, the sums relatively.  Prints one JSON line (and writes it to --out)."""
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


def reduce_on_host(labels, B, bins, dist):
    """The numpy reduction the baseline needs: sort the rows by their own label once, then segment reductions."""
    ok = (labels >= 0) & (labels < B)
    idx = np.flatnonzero(ok)
    order = idx[np.argsort(labels[idx], kind="stable")]
    own = labels[order]
    starts = np.searchsorted(own, np.arange(B))
    present = np.flatnonzero(np.diff(np.append(starts, len(own))) > 0)
    d = dist[order]
    fin = np.isfinite(d)
    dcnt = np.zeros((B, B), dtype=np.int64)
    dsum = np.zeros((B, B))
    dmin = np.full((B, B), np.inf)
    if len(present):
        at = starts[present]
        dcnt[present] = np.add.reduceat(fin.astype(np.int64), at, axis=0)
        dsum[present] = np.add.reduceat(np.where(fin, d, 0.0), at, axis=0)
        dmin[present] = np.minimum.reduceat(np.where(fin, d, np.inf), at, axis=0)
    bn = bins[order]
    placed = bn >= 0
    confusion = np.bincount(own[placed] * B + bn[placed], minlength=B * B).reshape(B, B)
    unplaced = np.bincount(own[~placed], minlength=B)
    return confusion, unplaced, dcnt, dmin, dsum, int(len(labels) - len(idx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=136)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--neighbors", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B, m = args.contigs, args.dim, args.bins, args.neighbors
    X, _, labels = synth.make_synthetic(N, D, B, seed=0)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    scored = int(np.count_nonzero((labels >= 0) & (labels < B)))
    ctx = _lib.Context(0)
    ctx.set_samples(X)

    def run_new():
        return ctx.bin_report(labels, B, m)

    def run_base():
        bins, dist, _, _ = ctx.audit_rows(labels, B, m)
        return reduce_on_host(labels, B, bins, dist)

    def note(what):
        print(f"[bin_report_bench] {what}", file=sys.stderr, flush=True)

    got = want = None
    for _ in range(args.warmup):
        got, want = run_new(), run_base()
        note("warm-up done")
    t_new, t_base, t_reduce = [], [], []
    for _ in range(args.repeats):   # alternating, same process
        t = time.perf_counter()
        got = run_new()
        t_new.append(time.perf_counter() - t)
        t = time.perf_counter()
        bins, dist, _, _ = ctx.audit_rows(labels, B, m)
        t1 = time.perf_counter()
        want = reduce_on_host(labels, B, bins, dist)
        t2 = time.perf_counter()
        t_base.append(t2 - t)
        t_reduce.append(t2 - t1)
        del bins, dist
        note(f"new {t_new[-1]:.3f} s, baseline {t_base[-1]:.3f} s")
    # kernel time: profiled repeats of their own
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(args.repeats):
        run_new()
    p_rep, p_aud = ctx.profile_get("bin_report"), ctx.profile_get("audit")
    ctx.profile_enable(False)

    tables = 4 * B * B * 8 + B * 8 + 8           # confusion, dcnt, dmin, dsum, unplaced, n_skipped
    up_new = scored * 4 + 8 * (min(B, scored) + -(-scored // 16384))   # sample indices + {label, start} of every run (at most)
    pos = want[4] > 0
    res = {
        "what": "chb_bin_report over all rows vs chb_audit_rows(dist_out) + numpy reduction",
        "contigs": N, "dim": D, "bins": B, "neighbors": m, "scored": scored, "warmup": args.warmup, "repeats": args.repeats,
        "new_wall_s": spread(t_new),
        "baseline_wall_s": spread(t_base),
        "baseline_numpy_reduction_s": spread(t_reduce),
        "baseline_over_new_wall": float(np.median(t_base) / np.median(t_new)),
        "new_not_slower": bool(np.median(t_new) <= np.median(t_base)),
        "new_bytes_down": tables, "new_bytes_up": up_new,
        "baseline_bytes_down": N * B * 8 + N * (4 + 8 + 8), "baseline_bytes_up": N * 4,
        "kernel_ms_per_call": {"audit": p_aud["ms"] / args.repeats, "bin_report": p_rep["ms"] / args.repeats},
        "launches_per_call": {"audit": p_aud["launches"] / args.repeats, "bin_report": p_rep["launches"] / args.repeats},
        "bin_report_share_of_device_time": p_rep["ms"] / (p_rep["ms"] + p_aud["ms"]) if p_rep["ms"] + p_aud["ms"] > 0 else None,
        "bin_report_pairs_per_s": p_rep["work"] / (p_rep["ms"] * 1e-3) if p_rep["ms"] > 0 else None,
        "same_counts_and_minima": bool(all(np.array_equal(got[i], want[i]) for i in (0, 1, 2, 3)) and got[5] == want[5]),
        "dsum_max_rel_difference": float((np.abs(got[4] - want[4])[pos] / want[4][pos]).max()) if pos.any() else 0.0,
        "rows_whose_bin_is_not_their_label": int(got[0].sum() - np.trace(got[0]) + got[1].sum()),
    }
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
