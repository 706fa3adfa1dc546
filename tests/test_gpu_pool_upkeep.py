"""Upkeep of the threshold pools by a batch's commit (prefilter_kernels.hip, pool_update_kernel).

A commit that the persistent pack served offers every bin the samples that ARRIVED in it from the tail of the bin's region
in the pack instead of looking for them in the batch's labels; a commit without the pack (CHB_PACK_INCR=0) keeps the scan.
Pools only set thresholds, so whole fits must equal a context without pools (CHB_POOL_TAU=0) and the oracle -- labels,
sweep counts, change counts, winning distances within the tolerance of test_gpu_parity's pools test -- and after the fit
every usable pool slot must be what the shortlist kernel relies on (the counter pool_bad_slots)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QP_TOL = 1e-9
D, M = 136, 5
POOLS = {"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}

# name: (generator settings, N, B, batch, sweeps)
CASES = {
    # an odd batch size (the tails of every 4- and 64-wide loop); from sweep 2 on the batches hold labelled samples:
    # holes, restores in place, leavers, arrivals
    "moves": (dict(sigma=6e-3, mix=0.5), 2500, 8, 257, 3),
    # about 256 arrivals of one bin in one commit: more than the 128 whose keys one pass gathers
    "many_arrivals": (dict(sigma=1.5e-3, mix=0.0), 4000, 4, 1024, 2),
    # bins that overlap almost wholly, five seeds each: sweep 1 puts most contigs into ONE bin (the oracle below: more than
    # 1500 of 2500), which outgrows the 544 rows (1.5 N / B + 64, in whole tiles) of its region several times over -- the
    # region moves, and that commit offers the bin's pools nothing
    "region_moves": (dict(sigma=6e-3, mix=0.9, n_seed=5), 2500, 8, 257, 2),
    # The fits of "moves" and "region_moves" drop their pools on the way (overlapping bins: long shortlists), after which
    # nobody keeps the pools up and pool_bad_slots has nothing to look at.  Slightly tighter bins keep them to the end, with
    # hundreds of contigs still moving in sweeps 2 and 3 and regions that move: the slot check sees pools that went through
    # holes, restores, leavers, arrivals and a moved bin
    "moves_pools_kept": (dict(sigma=5e-3, mix=0.5), 2500, 8, 257, 3),
}


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


_cache = {}


def _case(name):
    """The case's data, the oracle's fit and the fit of a context without pools: computed once, shared, left unchanged."""
    if name not in _cache:
        import chbin_amd
        from oracle import oracle as O
        gen, N, B, batch, sweeps = CASES[name]
        X, initial, _ = chbin_amd.synth.make_synthetic(N, D, B, seed=N + B, **gen)
        perms = chbin_amd.synth.draw_permutations(initial, sweeps, seed=0)
        want, its_o, ch_o = O.fit_cluster(X, B, initial, perms, M, sweeps)
        first, _ = O.sweep(X, B, initial, perms[0], M)
        b = _ctx_env({"CHB_POOL_TAU": "0", "CHB_TILE_SKIP": "0"})
        try:
            b.set_samples(X)
            ref, its_r, ch_r, mind_r = b.fit_cluster(B, initial, perms, M, sweeps, batch=batch, want_min_dist=True)
            assert b.counter("pool_batches") == 0 and b.counter("pool_bad_slots") == 0   # (no pools: nothing to check)
        finally:
            b.close()
        assert its_r == its_o and np.array_equal(ch_r, ch_o) and np.array_equal(ref, want)
        for a in (X, initial, perms, want, ch_o, first, mind_r):
            a.setflags(write=False)
        _cache[name] = dict(X=X, initial=initial, perms=perms, B=B, batch=batch, sweeps=sweeps, want=want, its=its_o, ch=ch_o,
                            first=first, mind=mind_r)
    return _cache[name]


def _fit_and_check(name, env):
    c = _case(name)
    names = ("pool_batches", "pool_state", "pack_incremental_batches", "pack_region_moves", "lookahead_batches", "lookahead_failed",
             "shortlist_short", "pool_bad_slots")
    a = _ctx_env(env)
    try:
        a.set_samples(c["X"])
        got, its, ch, mind = a.fit_cluster(c["B"], c["initial"], c["perms"], M, c["sweeps"], batch=c["batch"], want_min_dist=True)
        cnt = {k: a.counter(k) for k in names}
    finally:
        a.close()
    # the look-ahead path (the next batch's start is enqueued behind a gated commit); a context of its own: one whose fit
    # dropped the pools -- long shortlists on overlapping bins -- starts the same fit without them
    a = _ctx_env(env)
    try:
        a.set_samples(c["X"])
        got_t, its_t, ch_t = a.fit_cluster(c["B"], c["initial"], c["perms"], M, c["sweeps"], batch=c["batch"])
        cnt_t = {k: a.counter(k) for k in names}
    finally:
        a.close()
    print(name, env, cnt, cnt_t, "sweeps", its, "changed", list(ch))
    assert its == c["its"] and np.array_equal(ch, c["ch"]) and np.array_equal(got, c["want"])
    assert its_t == c["its"] and np.array_equal(ch_t, c["ch"]) and np.array_equal(got_t, c["want"])
    mv = c["initial"] < 0
    assert np.allclose(mind[mv], c["mind"][mv], rtol=0, atol=QP_TOL)
    assert cnt["pool_batches"] > 0 and cnt_t["pool_batches"] > 0
    assert cnt["shortlist_short"] == 0 and cnt_t["shortlist_short"] == 0
    assert cnt["pool_bad_slots"] == 0 and cnt_t["pool_bad_slots"] == 0
    return c, cnt, cnt_t


@pytest.mark.parametrize("name", ["moves", "many_arrivals"])
def test_pool_upkeep_from_the_packs_tails(name):
    c, cnt, _ = _fit_and_check(name, POOLS)
    assert cnt["pack_incremental_batches"] > 0
    if name == "moves":
        assert c["its"] >= 2 and c["ch"][1] > 0                         # labelled samples really moved after sweep 1
    else:
        arrivals = np.bincount(c["first"][c["perms"][0][:c["batch"]]], minlength=c["B"])
        assert arrivals.max() > 128, arrivals                           # one commit brought a bin more than one pass of keys


def test_pool_upkeep_slots_checked_on_pools_kept_to_the_end():
    c, cnt, cnt_t = _fit_and_check("moves_pools_kept", POOLS)
    assert cnt["pool_state"] == 1                                       # kept on: the slot check looked at live pools
    assert c["ch"][1] > 100 and c["ch"][2] > 100
    assert cnt["pack_incremental_batches"] > 0 and cnt["pack_region_moves"] > 0


def test_pool_upkeep_scan_form_without_the_pack():
    """(CHB_PACK_INCR=0: no batch is served by the persistent pack, so pack_incremental_batches is 0 here)"""
    _, cnt, _ = _fit_and_check("moves", dict(POOLS, CHB_PACK_INCR="0"))
    assert cnt["pack_incremental_batches"] == 0


def test_pool_upkeep_bin_whose_region_moves():
    c = _case("region_moves")
    N, B = c["X"].shape[0], c["B"]
    cap = (3 * N // 2 // B + 64 + 31) // 32 * 32
    assert np.bincount(c["first"][c["first"] >= 0], minlength=B).max() > cap    # (the oracle: sweep 1 collapses that far)
    _, cnt, cnt_t = _fit_and_check("region_moves", POOLS)
    assert cnt["pack_incremental_batches"] > 0
    assert cnt["pack_region_moves"] > 0 and cnt_t["pack_region_moves"] > 0
