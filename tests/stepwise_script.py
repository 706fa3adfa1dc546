"""The round script of the stepwise ABI tests: drives backends with the stepwise methods of chbin_amd._lib.Context
(fit_begin, batch_begin, batch_guess, batch_round, batch_commit) through rounds whose `lab_prev` the library's own loop
never produces.  The first backend is the reference (tests/oracle_backend.OracleBackend); every other backend gets the
same calls, and `compare(ref_record, record)` is called after every guess and round.  Test infrastructure only.

Rounds of one batch of K positions, slice [q_lo, q_hi):
    0   lab_prev = batch_guess of the last backend merged into the current labels        active 0
    1   random labels in [-1, B), about 10 % of them -1                                  active 0
    2   the same again (unchanged candidate sets: every kept distance must still hold)   active 0
    3   round 2 with three entries changed, one of them at a position < 10               active 10
    4.. the reference's round-3 result merged in, active = min(40, K // 2), and from there the driver rule of
        chbin_amd.distributed._sweeps until the batch converges
then the batch is committed on every backend.  Before every call the output arrays hold sentinels; the script itself
asserts that every backend leaves them alone outside [max(active, q_lo), q_hi) and overwrites them inside."""
import numpy as np

LAB_SENTINEL = -7
DIST_SENTINEL = -123.0
BATCH_SIZES = (96, 257, 40)     # 257: the batch buffers grow, no multiple of 16 or 64


def make_case(N, D, B, seed, unlabelled=0.3):
    """(X, initial, seeds mask): the generator's true labels with about `unlabelled` of the non-seed samples set to -1."""
    import chbin_amd
    X, seeds, true = chbin_amd.synth.make_synthetic(N, D, B, seed=seed, sigma=8e-3, mix=0.5)
    rng = np.random.default_rng(seed + 1000)
    initial = true.copy()
    initial[(rng.random(N) < unlabelled) & (seeds < 0)] = -1
    return X, initial, seeds >= 0


def draw_batches(is_seed, rng, sizes=BATCH_SIZES):
    """Each batch drawn from ALL non-seed samples: labelled and unlabelled ones mix, and samples of an earlier batch
    come back as base members or as entries."""
    pool = np.flatnonzero(~is_seed)
    return [rng.choice(pool, size=K, replace=False).astype(np.int64) for K in sizes]


def slices(K):
    """The four slice shapes: whole batch, uneven inner part (empty where the batch is too short for it), one position,
    empty at the end."""
    return {"full": (0, K), "inner": (17, max(K - 30, 17)), "one": (0, 1), "empty": (K, K)}


def _call_round(backends, lab_prev, active, lo, hi, B, compare, tag):
    """One round on every backend; returns the reference's (lab_new, min_dist)."""
    K = len(lab_prev)
    e_lo = min(max(int(active), lo), hi)
    recs = []
    for b in backends:
        lab_new = np.full(K, LAB_SENTINEL, dtype=np.int64)
        md = np.full(K, DIST_SENTINEL, dtype=np.float64)
        b.batch_round(lab_prev.copy(), int(active), lab_new, md)
        outside = np.ones(K, dtype=bool)
        outside[e_lo:hi] = False
        assert np.all(lab_new[outside] == LAB_SENTINEL) and np.all(md[outside] == DIST_SENTINEL), \
            f"{tag}: entries outside [{e_lo}, {hi}) were written"
        assert np.all((lab_new[e_lo:hi] >= -1) & (lab_new[e_lo:hi] < B)), f"{tag}: label out of range or not written"
        assert not np.any(md[e_lo:hi] == DIST_SENTINEL), f"{tag}: min_dist not written"
        recs.append({"kind": "round", "tag": tag, "lo": e_lo, "hi": hi, "lab_prev": lab_prev.copy(), "active": int(active),
                     "lab_new": lab_new, "min_dist": md, "all_dist": getattr(b, "all_dist", None)})
    if compare is not None:
        for r in recs[1:]:
            compare(recs[0], r)
    return recs[0]["lab_new"], recs[0]["min_dist"]


def run_batch(backends, sl, q_lo, q_hi, B, rng, compare=None, tag=""):
    """Runs the script on one batch.  Returns {"rounds": number of rounds, "active0": the `active` of round 4,
    "frozen": lab_prev[:active0] of round 4, "final": the committed labels}."""
    sl = np.asarray(sl, dtype=np.int64)
    K, lo, hi = len(sl), int(q_lo), int(q_hi)
    ref = backends[0]
    for b in backends:
        b.batch_begin(sl, lo, hi)
    cur = ref.labels[sl].copy()
    # ---- guess
    recs = []
    for b in backends:
        g = np.full(K, LAB_SENTINEL, dtype=np.int64)
        b.batch_guess(g)
        outside = np.ones(K, dtype=bool)
        outside[lo:hi] = False
        assert np.all(g[outside] == LAB_SENTINEL), f"{tag} guess: entries outside [{lo}, {hi}) were written"
        assert np.all((g[lo:hi] >= -1) & (g[lo:hi] < B)), f"{tag} guess: out of range or not written"
        recs.append({"kind": "guess", "tag": f"{tag} guess", "lo": lo, "hi": hi, "guess": g, "lab_old": cur.copy()})
    if compare is not None:
        for r in recs[1:]:
            compare(recs[0], r)
    lab0 = cur.copy()
    lab0[lo:hi] = recs[-1]["guess"][lo:hi]

    def rnd(n, lab_prev, active):
        new, _ = _call_round(backends, lab_prev, active, lo, hi, B, compare, f"{tag} round {n} active {active}")
        merged = lab_prev.copy()
        e_lo = min(max(int(active), lo), hi)
        merged[e_lo:hi] = new[e_lo:hi]
        return merged

    rnd(0, lab0, 0)
    r1 = rng.integers(0, B, size=K).astype(np.int64)
    r1[rng.random(K) < 0.1] = -1
    rnd(1, r1, 0)
    rnd(2, r1, 0)
    r3 = r1.copy()
    where = np.concatenate([rng.integers(0, 10, size=1), rng.choice(np.arange(10, K), size=2, replace=False)])
    r3[where] = (r3[where] + 1 + 1 + rng.integers(0, B, size=3)) % (B + 1) - 1     # (another value of [-1, B))
    assert np.all(r3[where] != r1[where])
    lab_prev = rnd(3, r3, 10)
    active = active0 = min(40, K // 2)
    frozen = lab_prev[:active0].copy()
    n = 4
    while True:                      # (the driver rule of chbin_amd.distributed._sweeps)
        lab_new = rnd(n, lab_prev, active)
        n += 1
        diff = np.flatnonzero(lab_new[active:] != lab_prev[active:])
        lab_prev[active:] = lab_new[active:]
        if diff.size == 0:
            break
        active = active + int(diff[0]) + 1      # positions <= first change are final
        if active >= K:
            break
    for b in backends:
        b.batch_commit(lab_prev)
    return {"rounds": n, "active0": active0, "frozen": frozen, "final": lab_prev.copy()}
