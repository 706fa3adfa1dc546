"""The m <= 5 fused kernel's trim (qp_kernels.hip, "Trim"; CHB_FUSED_TRIM=0 switches it off) in whole fits.

Each case is fitted by the developer library twice -- trim on and off, one child process each over all cases -- with every
one of the n_move x B hull distances of the last sweep dumped (CHB_DEV_ALL_DIST) and the shortlist stage's checks on.  Both
runs must return the oracle's labels, sweeps and change counts and its distances within QP_TOL (the pattern of
tests/test_gpu_bin_distances.py); between the two runs labels and counts are equal and the distances agree within 1e-12
relative (a Gram entry of a trimmed pair can be summed in another reduce-scatter slot, which may move its last bit).  The
largest difference seen on an MI355X: 6.3e-16 relative (affine case); the adversarial cases that keep everything: 0.

Shapes where wide shortlists are the rule: six seeds per bin, so sweep 1's batches are 1.5 x the labelled set and from
sweep 2 on the whole fit is ONE batch against 48 base members.  The trim's counters show that the route ran (and, for rows of
four shadow slices, that it did not).  The second group is data built to defeat the fp16 bound: identical members, a common
offset, tiny scale, a column with one huge outlier, one-hot rows."""
import numpy as np
import pytest

from test_gpu_bin_distances import QP_TOL, TINY, _run_child, oracle_replay

pytestmark = pytest.mark.gpu

TRIM_COUNTERS = ["fused_trim_pairs", "fused_trim_in", "fused_trim_kept", "fused_enabled", "prefilter_enabled",
                 "shortlist_short"]
SEEDS6 = dict(sigma=6e-3, mix=0.5, n_seed=6)
CASES = {
    "d136": dict(N=3000, D=136, B=8, m=5, its=3, batch=0, gen=SEEDS6),
    "d24": dict(N=3000, D=24, B=8, m=5, its=3, batch=0, gen=SEEDS6),
    "d141": dict(N=3000, D=141, B=8, m=5, its=3, batch=0, gen=SEEDS6),      # (Dz = 160)
    "m3": dict(N=3000, D=136, B=8, m=3, its=3, batch=0, gen=SEEDS6),
    "batch257": dict(N=3000, D=136, B=8, m=5, its=3, batch=257, gen=SEEDS6),
    "affine": dict(N=3000, D=136, B=8, m=5, its=3, batch=0, gen=SEEDS6, metric="affine"),
    # rows of four 144-column shadow slices: no trim
    "wide_d528": dict(N=1000, D=528, B=4, m=5, its=2, batch=0, gen=dict(sigma=6e-3, mix=0.5, n_seed=6), trims=False),
    # data built to defeat the bound
    "identical": dict(N=1500, D=136, B=4, m=5, its=2, batch=0, gen=SEEDS6, xform="identical", trims=None),
    "offset": dict(N=1500, D=136, B=4, m=5, its=2, batch=0, gen=SEEDS6, xform="offset", trims=None),
    "tiny": dict(N=1500, D=136, B=4, m=5, its=2, batch=0, gen=SEEDS6, xform="tiny", trims=None),
    "outlier": dict(N=1500, D=136, B=4, m=5, its=2, batch=0, gen=SEEDS6, xform="outlier", trims=None),
    "onehot": dict(N=1200, D=24, B=4, m=5, its=2, batch=0, gen=None, xform="onehot", trims=None),
}
NAMES = list(CASES)


def case_data(name):
    """(X, initial, perms) of a case; deterministic."""
    from chbin_amd import synth
    c = CASES[name]
    N, D, B = c["N"], c["D"], c["B"]
    xf = c.get("xform")
    if xf == "onehot":
        # bin c owns the columns 2 c and 2 c + 1; its first eight rows (four of each column) are its seeds: a contig is at
        # distance 0 from copies of itself and at exactly sqrt(2) from every other row
        i = np.arange(N)
        true = i % B
        X = np.zeros((N, D))
        X[i, 2 * true + (i // B) % 2] = 1.0
        initial = np.where(i < 8 * B, true, -1).astype(np.int64)
    else:
        X, initial, true = synth.make_synthetic(N, D, B, seed=N + D + B + c["m"], **c["gen"])
    mv = np.flatnonzero(initial < 0)
    if xf == "identical":
        # 300 identical members-to-be of bin 0: every bound ties
        ids = mv[true[mv] == 0][:300]
        X[ids] = X[ids[0]]
    elif xf == "offset":
        X = X + 1000.0
    elif xf == "tiny":
        X = X * TINY
    elif xf == "outlier":
        X[mv[5], 3] = 1e6   # S collapses: every shadow row rounds to zero or near it
    perms = synth.draw_permutations(initial, c["its"], seed=0)
    return np.ascontiguousarray(X), initial, perms


def replay(X, B, initial, perms, m, its, metric):
    """oracle_replay up to the sweep the reference stops at (its first sweep without a change)."""
    r = oracle_replay(X, B, initial, perms, m, its, metric)
    still = np.flatnonzero(r[2] == 0)
    return replay(X, B, initial, perms, m, int(still[0]) + 1, metric) if len(still) and still[0] + 1 < len(r[2]) else r


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Oracle replays (threads) and the two developer children."""
    import test_gpu_bin_distances as T
    from concurrent.futures import ThreadPoolExecutor
    tmp = tmp_path_factory.mktemp("fused_trim")
    data = {"_tmp": tmp}
    pool = ThreadPoolExecutor(max_workers=8)
    for name in NAMES:
        c = CASES[name]
        X, initial, perms = case_data(name)
        path = str(tmp / f"{name}.npz")
        np.savez(path, X=X, initial=initial, perms=perms)
        fut = pool.submit(replay, X, c["B"], initial, perms, c["m"], c["its"], c.get("metric", "convex"))
        data[name] = dict(X=X, initial=initial, perms=perms, npz=path, oracle=fut)
    saved = T.CASES, T.COUNTERS
    T.CASES, T.COUNTERS = CASES, TRIM_COUNTERS   # (_run_child reads its cases and counters from the module)
    try:
        on = _run_child(data, "trim_on", NAMES, {})
        off = _run_child(data, "trim_off", NAMES, {"CHB_FUSED_TRIM": "0"})
    finally:
        T.CASES, T.COUNTERS = saved
    yield data, on, off
    pool.shutdown(wait=False, cancel_futures=True)


def _against_oracle(name, d, run, what):
    rec, got, outs = run
    want, its_o, ch_o, alld = d["oracle"].result()
    assert rec["its"] == its_o and np.array_equal(outs["changed"], ch_o) and np.array_equal(outs["labels"], want), \
        (what, name, rec["its"], its_o, outs["changed"], ch_o)
    assert rec["counters"]["shortlist_short"] == 0 and rec["counters"]["fused_enabled"] == 1, (what, name, rec["counters"])
    mv = d["initial"] < 0
    assert np.all(np.isnan(got[~mv])) and not np.any(np.isnan(got[mv])), (what, name)
    g, o = got[mv], alld[mv]
    assert np.array_equal(np.isinf(g), np.isinf(o)), (what, name)
    fin = np.isfinite(o)
    err = np.abs(g[fin] - o[fin])
    bound = 1e-9 * np.abs(o[fin]) if CASES[name].get("xform") == "tiny" else QP_TOL
    assert np.all(err <= bound), (what, name, f"{int((err > bound).sum())} of {err.size} distances off, worst {err.max():.3g}")
    return err.max() if err.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_trim_on_and_off_equal_the_oracle_and_each_other(runs, name):
    data, on, off = runs
    d = data[name]
    worst_on = _against_oracle(name, d, on[name], "trim on")
    worst_off = _against_oracle(name, d, off[name], "trim off")
    (rec_on, got_on, outs_on), (rec_off, got_off, outs_off) = on[name], off[name]
    assert rec_on["its"] == rec_off["its"] and np.array_equal(outs_on["labels"], outs_off["labels"])
    assert np.array_equal(outs_on["changed"], outs_off["changed"])
    mv = d["initial"] < 0
    a, b = got_on[mv], got_off[mv]
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin)
    diff = np.abs(a[fin] - b[fin])
    rel = np.divide(diff, np.abs(b[fin]), out=np.where(diff == 0.0, 0.0, np.inf), where=b[fin] != 0.0)
    con, coff = rec_on["counters"], rec_off["counters"]
    print(f"\n{name}: {rec_on['its']} sweeps, {int(fin.sum())} finite distances; worst error against the oracle {worst_on:.3g} "
          f"(trim) / {worst_off:.3g} (no trim); trim on against off: worst relative difference {rel.max():.3g}; trim counters "
          f"pairs / in / kept = {con['fused_trim_pairs']} / {con['fused_trim_in']} / {con['fused_trim_kept']}")
    assert rel.max() <= 1e-12, (name, rel.max())
    assert coff["fused_trim_pairs"] == 0 and coff["fused_trim_in"] == 0, coff
    trims = CASES[name].get("trims", True)
    if trims is True:
        assert con["fused_trim_pairs"] > 0 and con["fused_trim_kept"] < con["fused_trim_in"], con
    elif trims is False:
        assert con["fused_trim_pairs"] == 0, con
