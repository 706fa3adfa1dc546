"""Every hull distance of whole fits against the oracle.

The label tests of test_gpu_parity.py see a hull distance only through the argmin over the bins: a distance that is wrong
for a bin that does not win -- or that wins anyway -- leaves the labels as they are.  Here each case's LAST sweep is
replayed by the oracle with all B distances of every visit (oracle.sweep(..., want_all=True), fp64 Goldfarb-Idnani), and

  (a) the product library (in process, chb_fit_cluster_ex) must return the oracle's labels, sweep and change counts, the
      row minimum as min_dist and second-smallest minus smallest as margin;
  (b) the developer library (child process) dumps the whole n_move x B matrix of the fit (CHB_DEV_ALL_DIST) with the
      shortlist stage's checks on (CHB_SL_BOUNDS, CHB_SL_VALIDATE): every entry must match the oracle's;
  (c) the same with the bins per workgroup of the shortlist launches forced (CHB_SL_BPW, read when a context is created:
      one child per value), above 64 once;
  (d) the ABI edges of margin_out.

The cases cover the shortlist builds the product uses (threshold pools, tile skipping, the persistent member pack, several
bins per workgroup), the hull kernels (fused m <= 5, 16-lane, wide rows, generic m > 16, list-based) and data edges.  A
counter of each fit shows that the build under test really ran."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QP_TOL = 1e-9
# scale of the scaled-data case (its distances are compared relative, to 1e-9).  Not 1e-150: there the Gram entries of the
# reference's QP form (2 X X^T, ~1e-300) multiply to below the fp64 range and the oracle's distances are off by ~3e-2
# relative to the enumerator's (from 1e-100 down); at 1e-50 they agree to ~3e-16 of the scale, like unscaled data
TINY = 1e-50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "ch-bin_amd", "libchbin_hip_dev.so")

# name: N, D, B, m, sweeps, batch (0 = default), generator keywords, product switches, expected counters
#   (counter, op, value); "bpw": also run with CHB_SL_BPW = 3 / above 64 (pool-forced cases)
CASES = {
    # threshold pools forced, the multi-bin pool build (no tile skipping), fused m = 5 kernel, odd batch, overlapping bins
    "pool_m5_batch257": dict(N=2500, D=136, B=8, m=5, its=2, batch=257, gen=dict(sigma=6e-3, mix=0.5),
                             env={"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}, expect=[("pool_batches", ">", 0)],
                             bpw=(3,)),
    # pools + tile skipping: five / ten coverage columns, m = 5 and the m = 8 (16-lane) builds
    "skip_pool_d140_m5": dict(N=6000, D=140, B=6, m=5, its=2, batch=512, gen=dict(S=5, sigma=2e-3, mix=0.2),
                              env={"CHB_POOL_TAU": "2"}, expect=[("tile_skipped", ">", 0), ("pool_batches", ">", 0)]),
    "skip_pool_d146_m8": dict(N=5000, D=146, B=5, m=8, its=2, batch=512, gen=dict(S=10, sigma=2e-3, mix=0.2),
                              env={"CHB_POOL_TAU": "2"}, expect=[("tile_seen", ">", 0), ("pool_batches", ">", 0)]),
    # the persistent member pack; in the developer child rebuilt at every batch start (CHB_PACK_REBUILD_AT=1)
    "pack_pressure": dict(N=3000, D=136, B=8, m=5, its=3, batch=400, gen=dict(sigma=6e-3, mix=0.5, n_seed=10),
                          env={"CHB_TILE_SKIP": "0"}, dev_env={"CHB_PACK_REBUILD_AT": "1"},
                          expect=[("pack_builds", ">", 10)]),
    # 16-lane kernel with the fp64 matrix-core tile: m = 15, and m = 16 with duplicated members (ties at the selection edge)
    "f16_m15": dict(N=700, D=136, B=4, m=15, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=20),
                    expect=[("fused_enabled", "==", 1)]),
    "f16_m16_dups": dict(N=500, D=64, B=3, m=16, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=20), xform="dups",
                         expect=[("fused_enabled", "==", 1)]),
    # wide rows: two, four and four (the widest) 144-column slices
    "wide_d300_m8": dict(N=1200, D=300, B=4, m=8, its=2, batch=600, gen=dict(sigma=6e-3, mix=0.5),
                         expect=[("fused_enabled", "==", 1)]),
    "wide_d528_m5": dict(N=1000, D=528, B=4, m=5, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5),
                         expect=[("fused_enabled", "==", 1)]),
    "wide_d573_m12": dict(N=600, D=573, B=3, m=12, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5),
                          expect=[("fused_enabled", "==", 1)]),
    # generic one-wavefront-per-problem kernels (m > 16)
    "generic_m24": dict(N=360, D=64, B=3, m=24, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=30),
                        expect=[("fused_enabled", "==", 0)]),
    # list-based path (exact rescoring + hull kernel)
    "lists_m5": dict(N=1500, D=136, B=5, m=5, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5),
                     env={"CHB_FUSED": "0"}, expect=[("fused_enabled", "==", 0)]),
    "lists_m12": dict(N=600, D=136, B=4, m=12, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=20),
                      env={"CHB_FUSED": "0"}, expect=[("fused_enabled", "==", 0)]),
    # a bin of two members (fewer than m) and a bin without any (a +inf column)
    "small_and_empty_bins": dict(N=400, D=64, B=7, m=5, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=8),
                                 xform="small_bins", expect=[("fused_enabled", "==", 1)]),
    # scaled data: every feature times 1e-50 (compared relative to the distances)
    "scaled_1e-50": dict(N=1200, D=136, B=4, m=5, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5), xform="tiny",
                          expect=[("prefilter_enabled", "==", 1)]),
    "affine": dict(N=800, D=64, B=6, m=5, its=3, batch=0, gen=dict(sigma=8e-3, mix=0.5, n_seed=8), metric="affine",
                   expect=[("fused_enabled", "==", 1)]),
    # more than 64 bins: with CHB_SL_BPW above 64 one workgroup holds bins past the 64-bin pool mask
    "pool_b70_one_sweep": dict(N=1500, D=136, B=70, m=5, its=1, batch=0, gen=dict(sigma=3e-3, mix=0.2, n_seed=4),
                               env={"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}, expect=[("pool_batches", ">", 0)],
                               bpw=(3, 80)),
}
NAMES = list(CASES)
COUNTERS = ["pool_batches", "pool_state", "tile_skip_state", "tile_skipped", "tile_seen", "tile_unloaded", "pack_builds",
            "pack_incremental_batches", "fused_enabled", "prefilter_enabled", "shortlist_short", "batch_size"]


def case_data(name):
    """(X, initial, perms) of a case; deterministic."""
    from chbin_amd import synth
    c = CASES[name]
    N, D, B = c["N"], c["D"], c["B"]
    gen = dict(c["gen"])
    X, initial, true = synth.make_synthetic(N, D, B, seed=N + D + B + c["m"], **gen)
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


def _min2(d):
    """Row minimum and second-smallest entry (the argmin kernel's winner and runner-up), NaN rows kept NaN."""
    s = np.sort(d, axis=1)
    return s[:, 0], s[:, 1] if d.shape[1] > 1 else np.full(len(d), np.inf)


def _margin(best, second):
    with np.errstate(invalid="ignore"):
        return np.where(second == np.inf, np.inf, second - best)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Every case's data (also written for the developer children) and its oracle replay, running on up to 8 threads
    (the oracle is a ctypes library: each call drops the GIL) while the GPU tests go on."""
    tmp = tmp_path_factory.mktemp("bin_distances")
    out = {}
    pool = ThreadPoolExecutor(max_workers=8)
    for name in NAMES:
        c = CASES[name]
        X, initial, perms = case_data(name)
        path = str(tmp / f"{name}.npz")
        np.savez(path, X=X, initial=initial, perms=perms)
        fut = pool.submit(oracle_replay, X, c["B"], initial, perms, c["m"], c["its"], c.get("metric", "convex"))
        out[name] = dict(X=X, initial=initial, perms=perms, npz=path, oracle=fut)
    out["_tmp"] = tmp
    yield out
    pool.shutdown(wait=False, cancel_futures=True)


def _oracle(data, name):
    return data[name]["oracle"].result()


def _ctx_env(env):
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


def _check_counters(name, cnt):
    ops = {">": lambda a, b: a > b, "==": lambda a, b: a == b}
    for k, op, v in CASES[name]["expect"]:
        assert ops[op](cnt[k], v), (name, k, cnt[k], op, v)


@pytest.mark.parametrize("name", NAMES)
def test_product_min_dist_and_margin(data, name):
    """(a) product library: labels, sweeps and changes equal the oracle's; min_dist is the row minimum of the oracle's
    distances and margin second-smallest minus smallest (0 on ties, +inf without a runner-up); seeds are NaN."""
    c, d = CASES[name], data[name]
    ctx = _ctx_env(c.get("env", {}))
    try:
        ctx.set_samples(d["X"])
        if c.get("metric"):
            ctx.set_metric(c["metric"])
        lab, its, ch, mind, margin = ctx.fit_cluster_margins(c["B"], d["initial"], d["perms"], c["m"], c["its"],
                                                            batch=c["batch"], want_min_dist=True)
        assert ctx.counter("shortlist_short") == 0
        cnt = {k: ctx.counter(k) for k in COUNTERS}
    finally:
        ctx.close()
    want, its_o, ch_o, alld = _oracle(data, name)
    assert its == its_o and np.array_equal(ch, ch_o) and np.array_equal(lab, want), (name, its, its_o, ch, ch_o)
    mv = d["initial"] < 0
    assert np.all(np.isnan(mind[~mv])) and np.all(np.isnan(margin[~mv]))
    best, second = _min2(alld[mv])
    tol = 1e-9 * np.abs(best) if c.get("xform") == "tiny" else QP_TOL
    assert np.array_equal(np.isinf(mind[mv]), np.isinf(best))
    fin = np.isfinite(best)
    assert np.all(np.abs(mind[mv] - best)[fin] <= (tol[fin] if np.ndim(tol) else tol)), name
    want_margin = _margin(best, second)
    assert np.array_equal(np.isinf(margin[mv]), np.isinf(want_margin)) and not np.any(np.isnan(margin[mv]))
    fin = np.isfinite(want_margin)
    tol_m = 2e-9 * np.maximum(np.abs(best), np.abs(second)) if c.get("xform") == "tiny" else 2 * QP_TOL
    assert np.all(np.abs(margin[mv] - want_margin)[fin] <= (tol_m[fin] if np.ndim(tol_m) else tol_m)), name
    print(f"\n[a] {name}: {its} sweeps, {int(mv.sum())} movable x {c['B']} bins, min margin "
          f"{np.min(margin[mv]):.3g}; counters {cnt}")


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


def _run_child(data, tag, names, env):
    """One developer-library child over `names` (contexts one after another, each with its case's switches); returns
    {name: (result record, dumped N x B distances, outputs)}."""
    if not os.path.exists(DEV_LIB):
        pytest.fail("developer library not built (__graft_entry__.build() makes it)")
    tmp = data["_tmp"]
    cases = []
    for name in names:
        c = CASES[name]
        cases.append(dict(name=name, npz=data[name]["npz"], B=c["B"], m=c["m"], its=c["its"], batch=c["batch"],
                          metric=c.get("metric"), env=dict(c.get("env", {})),
                          dump=str(tmp / f"{tag}_{name}.f64"), out=str(tmp / f"{tag}_{name}_out.npz")))
    job = dict(root=ROOT, cases=cases, counters=COUNTERS, result=str(tmp / f"{tag}.json"))
    (tmp / f"{tag}_job.json").write_text(json.dumps(job))
    (tmp / "child.py").write_text(CHILD)
    e = dict(os.environ, CHBIN_LIB=DEV_LIB, CHB_SL_BOUNDS="1", CHB_SL_VALIDATE="1", **env)
    p = subprocess.run([sys.executable, str(tmp / "child.py"), str(tmp / f"{tag}_job.json")], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads((tmp / f"{tag}.json").read_text())
    out = {}
    for c in cases:
        N, B = CASES[c["name"]]["N"], c["B"]
        alld = np.fromfile(c["dump"], dtype=np.float64)
        assert alld.size == N * B, (c["name"], alld.size)
        out[c["name"]] = (res[c["name"]], alld.reshape(N, B), dict(np.load(c["out"])))
    return out


@pytest.fixture(scope="module")
def dev_runs(data):
    """The developer children, one after another: the main one over every case except the pack case; the pack case with
    its rebuild mark (read when a context is created); then the bins-per-workgroup children."""
    runs = {}
    main = [n for n in NAMES if "dev_env" not in CASES[n]]
    runs["dev"] = _run_child(data, "dev", main, {})
    for n in NAMES:
        if "dev_env" in CASES[n]:
            runs["dev"].update(_run_child(data, "dev_" + n, [n], CASES[n]["dev_env"]))
    for bpw in (3, 80):
        names = [n for n in NAMES if bpw in CASES[n].get("bpw", ())]
        runs[f"bpw{bpw}"] = _run_child(data, f"bpw{bpw}", names, {"CHB_SL_BPW": str(bpw)})
    return runs


def _check_all_distances(data, name, rec, got, outs, what):
    c, d = CASES[name], data[name]
    want, its_o, ch_o, alld = _oracle(data, name)
    assert rec["its"] == its_o and np.array_equal(outs["changed"], ch_o) and np.array_equal(outs["labels"], want), \
        (what, name, rec["its"], its_o)
    assert rec["counters"]["shortlist_short"] == 0, (what, name)
    _check_counters(name, rec["counters"])
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
    best, second = _min2(g)
    assert np.array_equal(outs["mind"][mv], best), (what, name)
    assert np.array_equal(outs["margin"][mv], _margin(best, second))
    return err.max() if err.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_dev_all_distances(data, dev_runs, name):
    """(b) developer library, all n_move x B hull distances of the last sweep against the oracle: finite entries within
    1e-9 (relative 1e-9 for the scaled data), +inf exactly where the oracle has +inf; shortlist checks clean."""
    rec, got, outs = dev_runs["dev"][name]
    worst = _check_all_distances(data, name, rec, got, outs, "dev")
    extra = " (pack rebuilt at every batch start: CHB_PACK_REBUILD_AT=1)" if "dev_env" in CASES[name] else ""
    print(f"\n[b] {name}: {int(np.isfinite(got).sum())} finite + {int(np.isinf(got).sum())} +inf distances, worst "
          f"error {worst:.3g}; counters {rec['counters']}{extra}")


@pytest.mark.parametrize("bpw,name", [(b, n) for b in (3, 80) for n in NAMES if b in CASES[n].get("bpw", ())])
def test_dev_all_distances_forced_bins_per_workgroup(data, dev_runs, bpw, name):
    """(c) the same with CHB_SL_BPW forcing the bins per workgroup of the shortlist launches (no counter reports it: the
    value is the one set); 80 > 64 puts bins past the pools' 64-bin mask into one workgroup."""
    if bpw > 64:
        assert CASES[name]["B"] > 64
    rec, got, outs = dev_runs[f"bpw{bpw}"][name]
    worst = _check_all_distances(data, name, rec, got, outs, f"bpw{bpw}")
    print(f"\n[c] {name}: CHB_SL_BPW={bpw} (forced), worst error {worst:.3g}; counters {rec['counters']}")


def test_margin_abi_edges():
    """(d) chb_fit_cluster_ex: margin_out without min_dist_out is CHB_EINVAL; one bin gives +inf margins; a sweep where
    no bin has a member gives +inf distances and +inf margins (not inf - inf); seeds are NaN in both outputs."""
    import ctypes as C

    from chbin_amd import _lib, synth
    lib = _lib.load()
    X, initial, _ = synth.make_synthetic(300, 64, 1, seed=3, sigma=6e-3, n_seed=20)
    perms = synth.draw_permutations(initial, 2, seed=0)
    ctx = _lib.Context(0)
    try:
        ctx.set_samples(X)
        N = len(X)
        out = np.empty(N, dtype=np.int64)
        changed = np.zeros(2, dtype=np.int64)
        its = C.c_int(0)
        margin = np.empty(N)
        rc = lib.chb_fit_cluster_ex(ctx._h, 1, initial, perms, perms.shape[1], 5, 2, 0, out, C.byref(its), changed,
                                    None, margin.ctypes.data)
        assert rc == -1   # CHB_EINVAL
        # B = 1: nobody else to lose to
        lab, n_its, ch, mind, margin = ctx.fit_cluster_margins(1, initial, perms, 5, 2, want_min_dist=True)
        mv = initial < 0
        assert np.all(lab == 0) and np.all(np.isfinite(mind[mv])) and np.all(margin[mv] == np.inf)
        assert np.all(np.isnan(mind[~mv])) and np.all(np.isnan(margin[~mv]))
        # no member anywhere: every hull is empty, labels stay -1
        init0 = np.full(N, -1, dtype=np.int64)
        p0 = synth.draw_permutations(init0, 1, seed=0)
        lab, n_its, ch, mind, margin = ctx.fit_cluster_margins(3, init0, p0, 5, 1, want_min_dist=True)
        assert np.all(lab == -1) and n_its == 1 and ch[0] == 0
        assert np.all(mind == np.inf) and np.all(margin == np.inf)
    finally:
        ctx.close()
