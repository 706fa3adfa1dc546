#!/usr/bin/env python3
"""What a library enqueues and computes over a fixed list of small fits and queries, one JSON line per step: launch count
and work units of every profile name, every chb_counter, fit_stats, a hash of the labels and of the min_dist bytes.

A host-side change of chb_api.hip (batch_begin_dev, the round paths, the fit driver) must leave the output byte for byte as
it was: run it once per library (CHBIN_LIB=<path> selects one) and compare the two files.  The contexts are created under
the product switches one at a time, the way the tests' _ctx_env helpers do (chb_create reads them).  Exits non-zero if the
list as a whole misses a branch of the batch open (MUST_BE_SEEN)."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chbin_amd  # noqa: E402,F401
from chbin_amd import _lib, synth  # noqa: E402

PROFILE_NAMES = ("argmin", "bucket", "fit_start", "hull_qp", "pool", "prefilter", "prefilter_retry", "prefilter_update",
                 "query_norms", "rescore", "rescore_update", "slow_path", "topm_base", "topm_fallback", "topm_update")
COUNTERS = ("prefilter_overflow", "lookahead_batches", "lookahead_failed", "exchanges", "pack_incremental_batches",
            "pack_builds", "pool_batches", "pool_state", "pool_candidates", "pool_pairs", "shortlist_short",
            "shortlist_sum_last_batch", "shortlist_max_last_batch", "slow_pairs_last_round", "fused_enabled",
            "segment_batches", "batch_size", "tile_skip_state", "tile_skipped", "tile_seen", "tile_unloaded", "last_batch_k",
            "prefilter_enabled")
MUST_BE_SEEN = ("pack_incremental_batches", "pack_builds", "pool_batches", "segment_batches", "tile_seen",
                "lookahead_batches", "lookahead_failed", "launches:prefilter_retry", "launches:rescore", "launches:topm_base")

# name, switches, (N, D, B, m), make_synthetic keywords, sweeps, batch, extra step ("topm": a chb_topm_per_bin query under
# the final labels; "stepwise": one batch driven through chb_batch_begin / round / commit)
CASES = [
    ("odd_wide300", {}, (400, 300, 3, 5), dict(seed=303, sigma=6e-3, mix=0.5, n_seed=3), 4, 150, None),
    ("odd_many_bins", {}, (900, 146, 40, 5), dict(S=10, seed=186, sigma=6e-3, mix=0.5, n_seed=3), 4, 150, None),
    ("odd_m15", {}, (700, 200, 4, 15), dict(seed=204, sigma=6e-3, mix=0.5, n_seed=3), 4, 150, "topm"),
    ("m20", {}, (600, 64, 4, 20), dict(seed=21, sigma=8e-3, mix=0.5, n_seed=24), 2, 200, None),
    ("lookahead", {}, (6000, 136, 12, 5), dict(seed=7, sigma=1.5e-3, mix=0.0), 3, 512, "stepwise"),
    # overlapping bins in small batches (the data of tests/test_gpu_world2.py's SCHED_DATA): look-aheads that fail, so that
    # the host state saved where the window opened is put back
    ("lookahead_fails", {}, (3000, 136, 8, 5), dict(S=1, seed=3008, sigma=4.5e-3, mix=0.4, n_seed=8), 3, 32, None),
    ("pack", {"CHB_TILE_SKIP": "0"}, (6000, 136, 12, 5), dict(seed=6012, sigma=6e-3, mix=0.5, n_seed=12), 4, 512, None),
    ("pack_m15", {"CHB_TILE_SKIP": "0"}, (2500, 140, 9, 15), dict(S=5, seed=2509, sigma=4e-3, mix=0.3, n_seed=20), 3, 400, None),
    ("pack_off", {"CHB_TILE_SKIP": "0", "CHB_PACK_INCR": "0"}, (2500, 136, 9, 5), dict(seed=2509, sigma=4e-3, mix=0.3), 3, 400, None),
    ("pools", {"CHB_POOL_TAU": "2"}, (5000, 136, 8, 5), dict(seed=5008, sigma=2e-3, mix=0.2), 3, 512, "topm"),
    ("pools_pack", {"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}, (5000, 136, 8, 8), dict(seed=5008, sigma=2e-3, mix=0.2), 3, 512, None),
    ("pools_off", {"CHB_POOL_TAU": "0"}, (5000, 136, 8, 5), dict(seed=5008, sigma=2e-3, mix=0.2), 3, 512, None),
    ("tile_skip", {}, (4800, 140, 8, 5), dict(S=5, seed=11, sigma=2e-3, mix=0.2), 3, 1024, None),
    ("giant_bin", {"CHB_TILE_SKIP": "0"}, (8000, 136, 24, 5), dict(seed=5, sigma=2e-3, mix=0.2), 2, 1024, "topm"),
    ("giant_bin_no_seg", {"CHB_SEGMENTS": "0"}, (8000, 136, 24, 5), dict(seed=5, sigma=2e-3, mix=0.2), 2, 1024, None),
    ("brute", {"CHB_PREFILTER": "0"}, (900, 136, 6, 5), dict(seed=9, sigma=5e-3, mix=0.3, n_seed=6), 3, 256, "topm"),
    ("lists", {"CHB_FUSED": "0"}, (2500, 136, 9, 5), dict(seed=2509, sigma=4e-3, mix=0.3), 3, 400, "stepwise"),
]


def ctx_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def report(ctx, case, step, seen, **results):
    prof = {n: ctx.profile_get(n) for n in PROFILE_NAMES}
    rec = {"case": case, "step": step,
           "profile": {n: [p["launches"], p["work"]] for n, p in prof.items()},
           "counters": {n: ctx.counter(n) for n in COUNTERS}, "fit_stats": ctx.fit_stats(), **results}
    for n in MUST_BE_SEEN:
        seen[n] = seen.get(n, 0) + (prof[n[9:]]["launches"] if n.startswith("launches:") else rec["counters"][n])
    print(json.dumps(rec, sort_keys=True), flush=True)
    ctx.profile_reset()


def stepwise_batch(ctx, B, initial, m, K=300):
    """One batch of K unlabelled samples: guess, rounds until nothing changes (at most six), commit."""
    sl = np.flatnonzero(initial < 0)[:K].astype(np.int64)
    ctx.fit_begin(B, initial, m)
    ctx.batch_begin(sl, 0, len(sl))
    lab = np.zeros(len(sl), dtype=np.int64)
    ctx.batch_guess(lab)
    out, md, hashes = np.zeros_like(lab), np.zeros(len(sl)), []
    for _ in range(6):
        ctx.batch_round(lab, 0, out, md)
        hashes.append(digest(out, md))
        if np.array_equal(out, lab):
            break
        lab = out.copy()
    ctx.batch_commit(out)
    return {"rounds": hashes, "labels": digest(ctx.fit_labels())}


def main():
    seen = {}
    for name, env, (N, D, B, m), kw, sweeps, batch, extra in CASES:
        X, initial, _ = synth.make_synthetic(N, D, B, **kw)
        if name.startswith("giant_bin"):   # 18 of the 24 clusters under one label: a bin far larger than the rest
            remap = np.array([0] * 18 + [1, 2, 3, 4, 5, 6])
            B, initial = 7, np.where(initial >= 0, remap[np.maximum(initial, 0)], -1).astype(np.int64)
        perms = synth.draw_permutations(initial, sweeps, seed=0)
        ctx = ctx_env(env)
        try:
            ctx.profile_enable(1)
            ctx.set_samples(X)
            ctx.profile_reset()
            lab, its, ch, mind = ctx.fit_cluster(B, initial, perms, m, sweeps, batch=batch, want_min_dist=True)
            report(ctx, name, "fit_min_dist", seen, sweeps=its, changed=ch.tolist(), labels=digest(lab),
                   min_dist=digest(mind[initial < 0]))
            lab2, its2, ch2 = ctx.fit_cluster(B, initial, perms, m, sweeps, batch=batch)   # (the look-ahead may engage)
            report(ctx, name, "fit", seen, sweeps=its2, changed=ch2.tolist(), labels=digest(lab2))
            if extra == "topm":
                q = np.flatnonzero(initial < 0)[:200]
                idx, dist, cnt = ctx.topm_per_bin(lab, B, m, q)
                pad = np.arange(m)[None, None, :] >= cnt[:, :, None]   # (entries beyond a list's length are not results)
                report(ctx, name, "topm_per_bin", seen, lists=digest(np.where(pad, 0, idx), np.where(pad, 0.0, dist), cnt))
            elif extra == "stepwise":
                report(ctx, name, "stepwise", seen, **stepwise_batch(ctx, B, initial, m))
        finally:
            ctx.close()
    missing = [n for n in MUST_BE_SEEN if not seen.get(n)]
    if missing:
        print("the list never reached: " + ", ".join(missing), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
