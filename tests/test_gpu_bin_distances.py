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
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fit_replay as R
# the replay and the two checks live in fit_replay.py (shared with test_gpu_fit_neighbors.py); other modules of the suite
# take these names from here
from fit_replay import CHILD, DEV_LIB, QP_TOL, ROOT, TINY, oracle_replay  # noqa: F401
from fit_replay import ctx_env as _ctx_env, margin as _margin, min2 as _min2  # noqa: F401

pytestmark = pytest.mark.gpu

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
COUNTERS = list(R.COUNTERS)


def case_data(name):
    """(X, initial, perms) of a case; deterministic."""
    return R.case_data(CASES[name])


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


@pytest.mark.parametrize("name", NAMES)
def test_product_min_dist_and_margin(data, name):
    """(a) product library: labels, sweeps and changes equal the oracle's; min_dist is the row minimum of the oracle's
    distances and margin second-smallest minus smallest (0 on ties, +inf without a runner-up); seeds are NaN."""
    R.check_product(name, CASES[name], data[name], _oracle(data, name), COUNTERS)


def _run_child(data, tag, names, env):
    """One developer-library child over `names` (contexts one after another, each with its case's switches); returns
    {name: (result record, dumped N x B distances, outputs)}.  Cases and counters are this module's at the time of the
    call."""
    return R.run_child(data, tag, names, env, CASES, COUNTERS)


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
    return R.check_all_distances(name, CASES[name], data[name], _oracle(data, name), rec, got, outs, what)


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
