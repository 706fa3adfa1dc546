#!/usr/bin/env python3
"""Speed of chb_recruit_rows against what the library could do for the same question before it existed.

Question: the hull distance of Q NEW rows to every bin of a frozen labelling of N resident samples (default: the data of
BASELINE configs[2] -- N = 100k, D = 136, B = 64, m = 5 -- and Q = 20 000 rows of the same generator that are not samples).

  new       Context.recruit_rows(labels, B, m, Y) on a context that holds X
  baseline  a context that holds vstack(X, Y) with the rows of Y unlabelled: topm_per_bin for the rows of Y, then
            hull_distance_batch on the lists it returns

Both are timed the same way in this one process, alternating, after a warm-up of each: host wall-clock around calls that
end in a device synchronise, and for the new call the kernel time of chb_profile_get("recruit") from separate, profiled
repeats.  The baseline is reported twice: as the whole of what a caller had to do before the call existed, which begins
with set_samples(vstack(X, Y)) -- a fitted context holds X, not the stacked matrix -- and, the stricter comparison, the
two queries alone with the stacked matrix already resident.  The new call needs no upload but that of Y, which is inside
its window.  The two results are
compared entry by entry.  Prints one JSON line (and writes it to --out).

Roofline figure of the new kernel: the selection needs Q x (labelled samples) x D subtract / multiply / add triples in
fp64 VALU (three instructions: the sum must round like cdist's, so nothing is fused); the vector fp64 rate of an MI355X is
half its fp32 vector rate of 157.3 TFLOP/s, i.e. 78.6 TFLOP/s with an FMA counted as two, or 39.3e12 fp64 lane-instructions
per second."""
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
    ap.add_argument("--neighbors", type=int, default=5)
    ap.add_argument("--rows", type=int, default=20_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib, synth

    N, D, B, m, Q = args.contigs, args.dim, args.bins, args.neighbors, args.rows
    Z, _, true = synth.make_synthetic(N + Q, D, B, seed=0)
    X, Y = np.ascontiguousarray(Z[:N]), np.ascontiguousarray(Z[N:])
    labels = true[:N].copy()
    lab_ext = np.concatenate([labels, np.full(Q, -1, dtype=np.int64)])
    members = int(np.count_nonzero((labels >= 0) & (labels < B)))

    new = _lib.Context(0)
    t = time.perf_counter()
    new.set_samples(X)
    upload_new = time.perf_counter() - t
    base = None
    upload_base = None
    if not args.no_baseline:
        base = _lib.Context(0)
        t = time.perf_counter()
        base.set_samples(Z)
        upload_base = time.perf_counter() - t
    qidx = N + np.arange(Q, dtype=np.int64)

    def run_new():
        return new.recruit_rows(labels, B, m, Y)

    def run_base():
        idx, _, _ = base.topm_per_bin(lab_ext, B, m, qidx)
        d = base.hull_distance_batch(np.repeat(qidx, B), idx.reshape(Q * B, m))
        return d.reshape(Q, B)

    for _ in range(args.warmup):
        got = run_new()
        want = run_base() if base is not None else None
    t_new, t_base, t_base_up = [], [], []
    for _ in range(args.repeats):   # alternating, same process
        t = time.perf_counter()
        got = run_new()
        t_new.append(time.perf_counter() - t)
        if base is not None:
            t = time.perf_counter()
            base.set_samples(Z)
            t1 = time.perf_counter()
            want = run_base()
            t2 = time.perf_counter()
            t_base.append(t2 - t1)
            t_base_up.append(t2 - t)
    # kernel time: profiled repeats of their own
    new.profile_enable(True)
    new.profile_reset()
    for _ in range(args.repeats):
        run_new()
    prof = new.profile_get("recruit")
    new.profile_enable(False)
    kernel_s = prof["ms"] * 1e-3 / args.repeats

    triples = float(Q) * members * D
    res = {
        "what": "chb_recruit_rows vs set_samples(vstack) + topm_per_bin + hull_distance_batch",
        "contigs": N, "dim": D, "bins": B, "neighbors": m, "rows": Q, "labelled": members,
        "warmup": args.warmup, "repeats": args.repeats,
        "new_wall_s": spread(t_new),
        "new_kernel_s": kernel_s,
        "new_kernel_launches_per_call": prof["launches"] / args.repeats,
        "new_pairs_per_call": prof["work"] / args.repeats,
        "upload_new_s": upload_new,
        "selection_triples": triples,
        "triples_per_s": triples / kernel_s if kernel_s > 0 else None,
        "fp64_valu_fraction": 3.0 * triples / kernel_s / FP64_VALU_LANE_OPS if kernel_s > 0 else None,
        "fp64_valu_peak_lane_ops_per_s": FP64_VALU_LANE_OPS,
    }
    if base is not None:
        fin = np.isfinite(want)
        res.update({
            "baseline_queries_wall_s": spread(t_base),
            "baseline_with_set_samples_wall_s": spread(t_base_up),
            "upload_baseline_s": upload_base,
            "baseline_queries_over_new_wall": float(np.median(t_base) / np.median(t_new)),
            "baseline_with_set_samples_over_new_wall": float(np.median(t_base_up) / np.median(t_new)),
            "same_inf_pattern": bool(np.array_equal(fin, np.isfinite(got[1]))),
            "max_abs_difference": float(np.abs(got[1][fin] - want[fin]).max()) if fin.any() else 0.0,
            "same_bins": bool(np.array_equal(got[0], np.argmin(want, axis=1))),
        })
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    new.close()
    if base is not None:
        base.close()


if __name__ == "__main__":
    main()
