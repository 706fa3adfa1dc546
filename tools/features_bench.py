#!/usr/bin/env python3
"""Speed of chb_set_samples_from_sequences against what the library offered for the same job before it existed.

Job: contigs in, resident samples [k-mer blocks of a KmerK list | coverage columns] out (default: 20 000 contigs of 10 kb,
two coverage columns, the lists 4 / 4,5 / 3,4,5 -- 136, 648 and 680 k-mer columns).

  new  Context.set_samples_from_sequences(seqs, ks, extra=coverage): one upload of the sequence in chunks, one counting
       pass for the whole list, the matrix assembled on the device and made resident there
  old  one Context.kmer_frequencies(seqs, k) per k (each uploads the whole sequence and brings its block home), np.hstack
       with the coverage columns on the host, Context.set_samples of the result

Both run in this one process on one context, alternating, after a warm-up of each: host wall clock around calls that end
in a device synchronise (joining the sequences into one buffer is inside both windows), and the kernel time of
chb_profile_get("kmer_multi") / ("kmer_count") from separate, profiled repeats.  The two resident matrices are compared
through pairwise_distance of their first rows, and the old path's host matrix against return_matrix of the new one, for
equality.  Prints one JSON line per list (and writes them to --out)."""
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
    ap.add_argument("--contigs", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=10_000)
    ap.add_argument("--coverage-columns", type=int, default=2)
    ap.add_argument("--lists", default="4;4,5;3,4,5", help="KmerK lists, separated by ';'")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import chbin_amd  # noqa: F401
    from chbin_amd import _lib

    rng = np.random.default_rng(0)
    n, length, S = args.contigs, args.length, args.coverage_columns
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [lut[rng.integers(0, 4, size=length, dtype=np.uint8)].tobytes() for _ in range(n)]
    coverage = rng.random((n, S))
    coverage /= coverage.sum(axis=1, keepdims=True)
    bases = float(n) * length
    ctx = _lib.Context(0)
    lines = []
    for ks in [[int(k) for k in part.split(",")] for part in args.lists.split(";")]:
        def run_new(want=False):
            return ctx.set_samples_from_sequences(seqs, ks, extra=coverage, return_matrix=want)

        def run_old():
            X = np.hstack([ctx.kmer_frequencies(seqs, k) for k in ks] + [coverage])
            ctx.set_samples(X)
            return X

        for _ in range(args.warmup):
            run_new()
            run_old()
        t_new, t_old = [], []
        for _ in range(args.repeats):   # alternating, same process
            t = time.perf_counter()
            run_new()
            t_new.append(time.perf_counter() - t)
            t = time.perf_counter()
            run_old()
            t_old.append(time.perf_counter() - t)
        # kernel time: profiled repeats of their own
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            run_new()
            run_old()
        p_new, p_old = ctx.profile_get("kmer_multi"), ctx.profile_get("kmer_count")
        ctx.profile_enable(False)
        k_new, k_old = p_new["ms"] * 1e-3 / args.repeats, p_old["ms"] * 1e-3 / args.repeats
        # the same result
        X_old = run_old()
        d_old = ctx.pairwise_distance(0, 4)
        X_new = run_new(want=True)
        d_new = ctx.pairwise_distance(0, 4)
        res = {
            "what": "set_samples_from_sequences vs kmer_frequencies per k + hstack + set_samples",
            "ks": ks, "contigs": n, "length": length, "coverage_columns": S, "columns": int(X_new.shape[1]),
            "warmup": args.warmup, "repeats": args.repeats, "chunks": ctx.counter("kmer_chunks"),
            "new_wall_s": spread(t_new), "old_wall_s": spread(t_old),
            "old_over_new_wall": float(np.median(t_old) / np.median(t_new)),
            "new_kernel_s": k_new, "old_kernel_s": k_old,
            "new_kernel_launches_per_call": p_new["launches"] / args.repeats,
            "old_kernel_launches_per_call": p_old["launches"] / args.repeats,
            "new_gbase_per_s": bases / k_new / 1e9 if k_new > 0 else None,
            "old_gbase_per_s": bases * len(ks) / k_old / 1e9 if k_old > 0 else None,   # (every k reads every base)
            "same_matrix": bool(np.array_equal(X_old, X_new)),
            "same_resident_distances": bool(np.array_equal(d_old, d_new)),
        }
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
