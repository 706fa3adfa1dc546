"""Whole fits replayed by the oracle with every bin's hull distance, and the two checks built on the replay.

Shared by test_gpu_bin_distances.py (its cases: shortlist builds, kernels, data edges), test_gpu_fit_neighbors.py (one fit
per num_neighbors 1..17 on every route) and test_fit_neighbors_cpu.py (the condition that makes label equality a fair demand
of the latter, from the oracle alone).  A case is a dict

    N, D, B, m, its, batch (0 = default), gen (generator keywords), optional xform / metric, env (product switches read when
    a context is created), expect [(counter, op, value)]

and `data[name]` holds its X / initial / perms, the npz the developer children read and `oracle`, a future of
oracle_replay's result.

  check_product        (a) the product library in process: labels, sweeps, changes, min_dist, margin, NaN seeds
  run_child            one developer-library child over several cases (CHB_DEV_ALL_DIST, CHB_SL_BOUNDS, CHB_SL_VALIDATE)
  check_all_distances  (b) a child's n_move x B matrix of the last sweep against the oracle's, entry by entry
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

QP_TOL = 1e-9
# scale of the scaled-data case (its distances are compared relative, to 1e-9).  Not 1e-150: there the Gram entries of the
# reference's QP form (2 X X^T, ~1e-300) multiply to below the fp64 range and the oracle's distances are off by ~3e-2
# relative to the enumerator's (from 1e-100 down); at 1e-50 they agree to ~3e-16 of the scale, like unscaled data
TINY = 1e-50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "ch-bin_amd", "libchbin_hip_dev.so")

COUNTERS = ["pool_batches", "pool_state", "tile_skip_state", "tile_skipped", "tile_seen", "tile_unloaded", "pack_builds",
            "pack_incremental_batches", "fused_enabled", "prefilter_enabled", "shortlist_short", "batch_size"]


def case_data(c):
    """(X, initial, perms) of a case; deterministic.  The seed rule: N + D + B + m for the data (a case may name another
    `seed`, with its reason), 0 for the permutations."""
    from chbin_amd import synth
    N, D, B = c["N"], c["D"], c["B"]
    gen = dict(c["gen"])
    X, initial, true = synth.make_synthetic(N, D, B, seed=c.get("seed", N + D + B + c["m"]), **gen)
    xf = c.get("xform")
    if xf == "dups":
        rng = np.random.default_rng(1)
        X[rng.choice(N, N // 3, replace=False)] = X[rng.choice(N, N // 3, replace=False)]
    elif xf == "tiny":
        X = X * TINY
    elif xf == "small_bins":
        # bin B-2: two seeds taken from bin 0's seeds; bin B-1: no seed at all (the contigs the generator put there move)
        initial[initial == B - 2] = -1
        initial[initial == B - 1] = -1
        initial[np.flatnonzero(initial == 0)[:2]] = B - 2
    perms = synth.draw_permutations(initial, c["its"], seed=0)
    return np.ascontiguousarray(X), initial, perms


def oracle_replay(X, B, initial, perms, m, its, metric="convex"):
    """The reference loop over perms[:its] (algorithm.py:12-76), with ALL B hull distances of its last sweep's visits.
    Returns (labels, sweeps run, changes per sweep, N x B distances of the last sweep: NaN rows for the seeds)."""
    from oracle import oracle as O
    if its > 1:
        before, its_b, ch_b = O.fit_cluster(X, B, initial, perms[: its - 1], m, its - 1, metric=metric)
        if its_b < its - 1:   # (converged early: the reference's last sweep is sweep its_b)
            return oracle_replay(X, B, initial, perms, m, its_b, metric)
    else:
        before, ch_b = initial.copy(), np.zeros(0, dtype=np.int64)
    after, _, alld = O.sweep(X, B, before, perms[its - 1], m, want_all=True, metric=metric)
    full = np.full((len(X), B), np.nan)
    full[perms[its - 1]] = alld
    return after, its, np.append(ch_b, np.count_nonzero(after != before)), full


def oracle_all_sweeps(X, B, initial, perms, m, its, metric="convex"):
    """The same loop one sweep at a time, ALL B hull distances of EVERY sweep kept: a list of (labels before, labels after,
    N x B distances, NaN rows for the seeds), ending like the reference after its first sweep without a change.  Its last
    entry is what oracle_replay returns (test_fit_neighbors_cpu.py holds the two together)."""
    from oracle import oracle as O
    out, before = [], np.asarray(initial, dtype=np.int64).copy()
    for it in range(its):
        after, _, alld = O.sweep(X, B, before, perms[it], m, want_all=True, metric=metric)
        full = np.full((len(X), B), np.nan)
        full[perms[it]] = alld
        out.append((before, after, full))
        if np.array_equal(after, before):
            break
        before = after
    return out


def min2(d):
    """Row minimum and second-smallest entry (the argmin kernel's winner and runner-up), NaN rows kept NaN."""
    s = np.sort(d, axis=1)
    return s[:, 0], s[:, 1] if d.shape[1] > 1 else np.full(len(d), np.inf)


def margin(best, second):
    with np.errstate(invalid="ignore"):
        return np.where(second == np.inf, np.inf, second - best)


def ctx_env(env):
    """A context created with the switches `env` set (they are read when a context is created)."""
    from chbin_amd import _lib
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


def check_counters(name, c, cnt):
    ops = {">": lambda a, b: a > b, "==": lambda a, b: a == b}
    for k, op, v in c["expect"]:
        assert ops[op](cnt[k], v), (name, k, cnt[k], op, v)


def check_product(name, c, d, oracle, counters=COUNTERS):
    """(a) product library: labels, sweeps and changes equal the oracle's; min_dist is the row minimum of the oracle's
    distances and margin second-smallest minus smallest (0 on ties, +inf without a runner-up); seeds are NaN.  Returns
    (worst min_dist error, the fit's counters)."""
    ctx = ctx_env(c.get("env", {}))
    try:
        ctx.set_samples(d["X"])
        if c.get("metric"):
            ctx.set_metric(c["metric"])
        lab, its, ch, mind, marg = ctx.fit_cluster_margins(c["B"], d["initial"], d["perms"], c["m"], c["its"],
                                                          batch=c["batch"], want_min_dist=True)
        assert ctx.counter("shortlist_short") == 0
        cnt = {k: ctx.counter(k) for k in counters}
    finally:
        ctx.close()
    want, its_o, ch_o, alld = oracle
    assert its == its_o and np.array_equal(ch, ch_o) and np.array_equal(lab, want), (name, its, its_o, ch, ch_o)
    mv = d["initial"] < 0
    assert np.all(np.isnan(mind[~mv])) and np.all(np.isnan(marg[~mv]))
    best, second = min2(alld[mv])
    tol = 1e-9 * np.abs(best) if c.get("xform") == "tiny" else QP_TOL
    assert np.array_equal(np.isinf(mind[mv]), np.isinf(best))
    fin = np.isfinite(best)
    err = np.abs(mind[mv] - best)[fin]
    assert np.all(err <= (tol[fin] if np.ndim(tol) else tol)), (name, f"worst min_dist error {err.max():.3g}")
    want_margin = margin(best, second)
    assert np.array_equal(np.isinf(marg[mv]), np.isinf(want_margin)) and not np.any(np.isnan(marg[mv]))
    fin = np.isfinite(want_margin)
    tol_m = 2e-9 * np.maximum(np.abs(best), np.abs(second)) if c.get("xform") == "tiny" else 2 * QP_TOL
    assert np.all(np.abs(marg[mv] - want_margin)[fin] <= (tol_m[fin] if np.ndim(tol_m) else tol_m)), name
    print(f"\n[a] {name}: {its} sweeps, {int(mv.sum())} movable x {c['B']} bins, min margin "
          f"{np.min(marg[mv]):.3g}; counters {cnt}")
    return (err.max() if err.size else 0.0), cnt


CHILD = r"""
import json, os, sys
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
import numpy as np
import chbin_amd
from chbin_amd import _lib
res = {}
for c in job["cases"]:
    d = np.load(c["npz"])
    old = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        ctx = _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        ctx.set_samples(d["X"])
        if c["metric"]:
            ctx.set_metric(c["metric"])
        os.environ["CHB_DEV_ALL_DIST"] = c["dump"]
        try:
            lab, its, ch, mind, margin = ctx.fit_cluster_margins(c["B"], d["initial"], d["perms"], c["m"], c["its"],
                                                                batch=c["batch"], want_min_dist=True)
        finally:
            del os.environ["CHB_DEV_ALL_DIST"]
        cnt = {k: int(ctx.counter(k)) for k in job["counters"]}
    finally:
        ctx.close()
    np.savez(c["out"], labels=lab, changed=ch, mind=mind, margin=margin)
    res[c["name"]] = {"its": int(its), "counters": cnt}
    print(c["name"], its, cnt, flush=True)
json.dump(res, open(job["result"], "w"))
"""


def run_child(data, tag, names, env, cases, counters=COUNTERS, timeout=300):
    """One developer-library child over `names` (contexts one after another, each with its case's switches); returns
    {name: (result record, dumped N x B distances, outputs)}."""
    if not os.path.exists(DEV_LIB):
        pytest.fail("developer library not built (__graft_entry__.build() makes it)")
    tmp = data["_tmp"]
    jobs = []
    for name in names:
        c = cases[name]
        jobs.append(dict(name=name, npz=data[name]["npz"], B=c["B"], m=c["m"], its=c["its"], batch=c["batch"],
                         metric=c.get("metric"), env=dict(c.get("env", {})),
                         dump=str(tmp / f"{tag}_{name}.f64"), out=str(tmp / f"{tag}_{name}_out.npz")))
    job = dict(root=ROOT, cases=jobs, counters=counters, result=str(tmp / f"{tag}.json"))
    (tmp / f"{tag}_job.json").write_text(json.dumps(job))
    (tmp / "child.py").write_text(CHILD)
    e = dict(os.environ, CHBIN_LIB=DEV_LIB, CHB_SL_BOUNDS="1", CHB_SL_VALIDATE="1", **env)
    p = subprocess.run([sys.executable, str(tmp / "child.py"), str(tmp / f"{tag}_job.json")], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads((tmp / f"{tag}.json").read_text())
    out = {}
    for c in jobs:
        N, B = cases[c["name"]]["N"], c["B"]
        alld = np.fromfile(c["dump"], dtype=np.float64)
        assert alld.size == N * B, (c["name"], alld.size)
        out[c["name"]] = (res[c["name"]], alld.reshape(N, B), dict(np.load(c["out"])))
    return out


def check_all_distances(name, c, d, oracle, rec, got, outs, what):
    """(b) a developer child's dump against the oracle: labels, sweeps, changes and counters; every finite entry within
    QP_TOL (relative 1e-9 for the scaled data), +inf exactly where the oracle has it; the dumped rows' winner and runner-up
    are what min_dist and margin report.  Returns the worst error."""
    want, its_o, ch_o, alld = oracle
    assert rec["its"] == its_o and np.array_equal(outs["changed"], ch_o) and np.array_equal(outs["labels"], want), \
        (what, name, rec["its"], its_o)
    assert rec["counters"]["shortlist_short"] == 0, (what, name)
    check_counters(name, c, rec["counters"])
    mv = d["initial"] < 0
    assert np.all(np.isnan(got[~mv])) and not np.any(np.isnan(got[mv])), (what, name)
    g, o = got[mv], alld[mv]
    assert np.array_equal(np.isinf(g), np.isinf(o)), (what, name, np.argwhere(np.isinf(g) != np.isinf(o))[:8])
    fin = np.isfinite(o)
    err = np.abs(g[fin] - o[fin])
    bound = 1e-9 * np.abs(o[fin]) if c.get("xform") == "tiny" else QP_TOL
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (what, name, f"{bad.size} of {err.size} distances off, worst {err.max():.3g}")
    # the winner and runner-up of the dumped rows are what min_dist / margin report (and what (a) saw)
    best, second = min2(g)
    assert np.array_equal(outs["mind"][mv], best), (what, name)
    assert np.array_equal(outs["margin"][mv], margin(best, second))
    return err.max() if err.size else 0.0


# ---- one fit per num_neighbors: the cases of test_gpu_fit_neighbors.py and test_fit_neighbors_cpu.py ----------------------

M_ALL = tuple(range(1, 18))
POOL_SWITCHES = {"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}
# family: shape, generator, sweeps, batch and the m of its data sets
FAMILIES = {
    # every list is full from the first visit: 20 seeds per bin, m <= 17
    "full": dict(N=500, D=64, B=4, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=20), ms=M_ALL),
    # three seeds per bin and ONE sweep: for m >= 4 every bin starts below m members and grows past m in the compared sweep.
    # m = 4 takes the next seed (573): with the rule's 572 bin 2 wins no visit and ends the sweep with its three seeds
    "short": dict(N=500, D=64, B=4, its=1, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=3), ms=M_ALL, seeds={4: 573}),
    # ... and that data set (seed 572 by the rule) kept for what it is: a bin whose list is short of m at EVERY visit
    "stuck": dict(N=500, D=64, B=4, its=1, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=3), ms=(4,)),
    # shape and switches of test_gpu_bin_distances.py's pool_m5_batch257 (m = 5 is that case)
    "pools": dict(N=2500, D=136, B=8, its=2, batch=257, gen=dict(sigma=6e-3, mix=0.5), ms=(1, 2, 3, 4, 6, 7, 8, 9)),
}
# family -> route -> (switches, m of the route)
ROUTES = {
    "full": {"default": ({}, M_ALL), "lists": ({"CHB_FUSED": "0"}, M_ALL[:16])},
    "short": {"default": ({}, M_ALL), "lists": ({"CHB_FUSED": "0"}, M_ALL[:16])},
    "stuck": {"default": ({}, (4,)), "lists": ({"CHB_FUSED": "0"}, (4,))},
    "pools": {"pooled": (POOL_SWITCHES, FAMILIES["pools"]["ms"])},
}


def neighbor_expect(family, route, m):
    """The counters that prove which route a fit took; with m they determine the kernel (the table in
    test_gpu_fit_neighbors.py)."""
    if family == "pools":
        return [("pool_batches", ">", 0) if m <= 8 else ("pool_batches", "==", 0), ("fused_enabled", "==", 1)]
    if route == "lists":
        return [("fused_enabled", "==", 0), ("prefilter_enabled", "==", 1)]
    return [("prefilter_enabled", "==", 1), ("fused_enabled", "==", 1 if m <= 16 else 0)]


def neighbor_data_name(family, m):
    return f"{family}-m{m}"


def neighbor_data_case(family, m):
    """The case of a (family, m) data set and its oracle replay, shared by the family's routes."""
    f = FAMILIES[family]
    c = dict(N=f["N"], D=f["D"], B=f["B"], m=m, its=f["its"], batch=f["batch"], gen=dict(f["gen"]))
    if m in f.get("seeds", {}):
        c["seed"] = f["seeds"][m]
    return c


def neighbor_cases():
    """{"family-route-mM": case} in the order family, route, m."""
    out = {}
    for family, routes in ROUTES.items():
        for route, (env, ms) in routes.items():
            for m in ms:
                out[f"{family}-{route}-m{m}"] = dict(neighbor_data_case(family, m), family=family, route=route,
                                                     env=dict(env), expect=neighbor_expect(family, route, m))
    return out
