"""The keep rule of the m <= 5 fused kernel's trim (qp_kernels.hip, "Trim"), mirrored in numpy (tools/fused_trim_probe.py:
shadow rows through float16, rho exact): the kept set must contain every candidate within 1e-6 relative of the pair's m-th
exact distance -- on random data and on the inputs built to defeat the bound that tests/test_gpu_fused_trim.py runs on the
GPU.  And, before a GPU is asked: the first GPU shape really puts its pairs into the trim's class."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fused_trim_probe as P  # noqa: E402

synth = P.load_synth()
TINY = 1e-50


def adversarial(kind, rng):
    """(X, m): rows 1.. are one pair's candidates, row 0 the query."""
    n, D = 24, 136
    X, _, _ = synth.make_synthetic(400, D, 4, seed=7, sigma=6e-3, mix=0.5)
    if kind == "identical":
        X[1:n + 1] = X[1]
    elif kind == "offset":
        X = X + 1000.0
    elif kind == "tiny":
        X = X * TINY
    elif kind == "outlier":
        X[300, 3] = 1e6   # (not a candidate: it only collapses S)
    elif kind == "onehot":
        X = np.zeros_like(X)
        X[np.arange(len(X)), rng.integers(0, 6, len(X))] = 1.0
    return X, n


def check_pair(X, j, ids, m, mu, S, G, rho):
    keep = P.trim_keep(G[j], rho[j], G[ids], rho[ids], m)
    d = np.sqrt(((X[ids] - X[j]) ** 2).sum(axis=1))
    dm = np.sort(d)[m - 1]
    must = d <= dm * (1.0 + 1e-6)
    assert np.all(keep[must]), (j, d[must & ~keep], dm)
    assert keep.sum() >= m
    return int(keep.sum())


@pytest.mark.parametrize("m", [1, 3, 5])
def test_random_pairs_keep_the_m_nearest_and_their_ties(m):
    rng = np.random.default_rng(m)
    X, _, _ = synth.make_synthetic(2000, 136, 8, seed=1, sigma=6e-3, mix=0.5)
    mu, S = P.shadow_scale(X)
    G, rho = P.shadows(X, mu, S)
    dropped = 0
    for _ in range(300):
        n = int(rng.integers(8, 33))
        ids = rng.choice(len(X), n + 1, replace=False)
        dropped += n - check_pair(X, ids[0], ids[1:], m, mu, S, G, rho)
    assert dropped > 0   # (the rule is not vacuous on this data)


@pytest.mark.parametrize("kind", ["identical", "offset", "tiny", "outlier", "onehot"])
def test_adversarial_pairs(kind):
    rng = np.random.default_rng(3)
    X, n = adversarial(kind, rng)
    mu, S = P.shadow_scale(X)
    G, rho = P.shadows(X, mu, S)
    kept = [check_pair(X, 0, np.arange(1, n + 1), m, mu, S, G, rho) for m in (1, 3, 5)]
    for _ in range(50):
        ids = rng.choice(len(X), n + 1, replace=False)
        check_pair(X, ids[0], ids[1:], 5, mu, S, G, rho)
    if kind == "identical":
        assert kept == [n, n, n], kept   # every bound ties: nothing can be dropped
    # (outlier: S collapses to 2^-10 and the rows land among fp16's subnormals -- coarse bounds, covered by rho like any other)


def test_a_nan_keeps_everything():
    G = np.arange(36.0).reshape(9, 4)
    rho = np.zeros(9)
    assert not P.trim_keep(np.zeros(4), 0.0, G, rho, 5).all()
    assert P.trim_keep(np.array([np.nan, 0.0, 0.0, 0.0]), 0.0, G, rho, 5).all()
    assert P.trim_keep(np.zeros(4), np.nan, G, rho, 5).all()
    rho[3] = np.nan
    assert P.trim_keep(np.zeros(4), 0.0, G, rho, 5).all()


def test_first_gpu_shape_is_in_the_trim_class():
    """tests/test_gpu_fused_trim.py's first shape: by the candidate lists of the reference's own sweep 1 (exact distances,
    the driver's batches), at least 10 % of the sampled (position, bin) pairs have 7 < n <= 32 candidates."""
    from oracle import oracle as O
    from test_gpu_fused_trim import CASES
    c = CASES["d136"]
    X, initial, _ = synth.make_synthetic(c["N"], c["D"], c["B"], seed=c["N"] + c["D"] + c["B"] + c["m"], **c["gen"])
    perm = synth.draw_permutations(initial, 1, seed=0)[0]
    after = O.sweep(X, c["B"], initial.copy(), perm, c["m"])[0]
    mu, S = P.shadow_scale(X)
    rng = np.random.default_rng(0)
    lab = initial.copy()
    ns = []
    for t0, K in P.batches_of_sweep1(int((initial >= 0).sum()), len(perm)):
        base = np.flatnonzero(lab >= 0)
        batch = perm[t0:t0 + K]
        labb = lab.copy()
        labb[batch] = after[batch]
        for p in rng.choice(K, min(20, K), replace=False):
            ns += [len(ids) for ids in P.pair_candidates(X, labb, base, batch[:p], batch[p], c["B"], c["m"])]
        lab[batch] = after[batch]
    ns = np.array(ns)
    share = np.mean((ns > P.C_NARROW) & (ns <= P.TRIM_MAX))
    print(f"\n{len(ns)} pairs: mean n {ns.mean():.2f}, 7 < n <= 32: {100 * share:.1f} %, n > 32: {100 * np.mean(ns > 32):.1f} %")
    assert share >= 0.10, share
