"""Per-round parity of the stepwise ABI (chb_fit_begin, chb_batch_begin, chb_batch_guess, chb_batch_round,
chb_batch_commit, chb_fit_labels) with the CPU oracle, and chb_set_samples_device.

A batch ends when a round reproduces its input, so whole-fit tests see a round only at its fixed point.  Here every
round of tests/stepwise_script.py -- starts the library's own loop never produces, repeated and slightly changed
inputs for the cross-round shortcuts, uneven / one-element / empty slices, a growing batch buffer -- is compared with
tests/oracle_backend.OracleBackend, which states the round's definition: position `pos` is visited with the earlier
batch members at `lab_prev` and the later ones at their old label.  Labels must be equal, winning distances within
QP_TOL (+inf exactly), everything outside [max(active, q_lo), q_hi) untouched.

Wall time of the file on one MI355X: 8 s (16 tests; each case of test_every_round_equals_the_oracle 0.4 - 0.8 s, nearly all
of it the oracle, whose positions of a round are evaluated on up to 16 host threads)."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the process then runs one HIP runtime, torch's, as bench.py does)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stepwise_script as S  # noqa: E402
from oracle_backend import OracleBackend  # noqa: E402

pytestmark = pytest.mark.gpu

QP_TOL = 1e-9
TIE_TOL = 1e-7            # 100 x QP_TOL: an oracle runner-up this close to its best may flip the argmin
ORACLE_THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
MAX_LEFT_OUT = 0.005      # share of a case's compared positions the near-tie rule may leave out of the label comparison


@pytest.fixture(scope="module")
def ctx():
    import chbin_amd  # noqa: F401
    from chbin_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


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


# name -> (N, D, B, m), data seed, environment switches, metric, counters that prove the path, guess_kernel runs
CASES = {
    "fused5": ((600, 136, 5, 5), 11, None, "convex", {"fused_enabled": 1}, False),
    "fused16": ((500, 40, 4, 12), 12, None, "convex", {"fused_enabled": 1}, False),
    "fused16_m16": ((400, 64, 3, 16), 13, None, "convex", {"fused_enabled": 1}, False),
    "wide": ((500, 300, 3, 5), 14, None, "convex", {"prefilter_enabled": 1, "fused_enabled": 1}, False),
    "lists": ((600, 136, 4, 5), 15, {"CHB_FUSED": "0"}, "convex", {"fused_enabled": 0, "prefilter_enabled": 1}, True),
    "plain": ((400, 600, 3, 5), 16, None, "convex", {"prefilter_enabled": 0}, True),       # D > 573: no shortlist stage
    "generic": ((300, 24, 2, 20), 17, None, "convex", {"fused_enabled": 0}, True),
    # the stepwise entry points never run the threshold pools (they are kept up by chb_fit_cluster's loop alone): the
    # switches select the ordinary two-sweep shortlist launch here, and "pool_batches" stays 0
    "pools": ((2500, 136, 4, 5), 18, {"CHB_POOL_TAU": "2", "CHB_TILE_SKIP": "0"}, "convex", {"fused_enabled": 1}, False),
    "affine": ((500, 64, 4, 5), 19, None, "affine", {}, False),
    "small_bins": ((400, 64, 6, 5), 20, None, "convex", {}, False),
}


def _case_data(name):
    (N, D, B, m), seed = CASES[name][0], CASES[name][1]
    X, initial, is_seed = S.make_case(N, D, B, seed=seed)
    if name == "small_bins":
        initial = initial.copy()
        initial[initial == B - 1] = -1                          # one bin with no member at all
        initial[np.flatnonzero(initial == B - 2)[2:]] = -1      # one with two
        assert (initial == B - 1).sum() == 0 and (initial == B - 2).sum() == 2
    return X, initial, is_seed


class _Compare:
    """compare(reference record, record of the backend under test) of the round script."""

    def __init__(self, ref, B, exact_guess):
        self.ref, self.B, self.exact_guess = ref, B, exact_guess
        self.compared = self.left_out = self.rounds = 0
        self.empty_bin = None          # a bin without members that no entry of lab_prev names either

    def __call__(self, want, got):
        (self._guess if want["kind"] == "guess" else self._round)(want, got)

    def _guess(self, want, got):
        lo, hi, tag = want["lo"], want["hi"], got["tag"]
        g, old = got["guess"], want["lab_old"]
        outside = self.ref.labels.copy()
        outside[self.ref.sl] = -1
        has_member = np.array([(outside == c).any() for c in range(self.B)])
        for pos in range(lo, hi):
            if old[pos] >= 0:
                assert g[pos] == old[pos], f"{tag}: position {pos} had label {old[pos]}, guess {g[pos]}"
            elif has_member.any():
                assert g[pos] >= 0 and has_member[g[pos]], \
                    f"{tag}: position {pos} guessed bin {g[pos]}, which has no member outside the batch"
            else:
                assert g[pos] == -1, f"{tag}: position {pos} guessed bin {g[pos]}, no bin has a member"
        if self.exact_guess:
            bad = np.flatnonzero(g[lo:hi] != want["guess"][lo:hi])
            assert bad.size == 0, (f"{tag}: position {lo + bad[0]} guessed bin {g[lo + bad[0]]}, its nearest member "
                                   f"outside the batch is in bin {want['guess'][lo + bad[0]]}")

    def _round(self, want, got):
        lo, hi, tag = want["lo"], want["hi"], got["tag"]
        self.rounds += 1
        if hi <= lo:
            return
        wl, gl = want["lab_new"][lo:hi], got["lab_new"][lo:hi]
        wd, gd = want["min_dist"][lo:hi], got["min_dist"][lo:hi]
        alld = want["all_dist"][lo:hi]
        # ---- winning distances: every position, +inf exactly
        inf_w, inf_g = np.isposinf(wd), np.isposinf(gd)
        bad = np.flatnonzero(inf_w != inf_g)
        assert bad.size == 0, f"{tag}: position {lo + bad[0]} min_dist {gd[bad[0]]} vs oracle {wd[bad[0]]}"
        err = np.where(inf_w, 0.0, np.abs(np.where(inf_w, 0.0, gd) - np.where(inf_w, 0.0, wd)))
        assert not np.any(np.isnan(gd)), f"{tag}: NaN min_dist at position {lo + np.flatnonzero(np.isnan(gd))[0]}"
        bad = np.flatnonzero(err > QP_TOL)
        assert bad.size == 0, (f"{tag}: position {lo + bad[0]} (bin {gl[bad[0]]}, oracle bin {wl[bad[0]]}) min_dist "
                               f"{gd[bad[0]]!r} vs oracle {wd[bad[0]]!r}; {bad.size} of {hi - lo} positions off")
        # ---- labels: exact, but for positions where the oracle's own runner-up is within TIE_TOL of its best
        srt = np.sort(np.where(np.isnan(alld), np.inf, alld), axis=1)
        best = srt[:, 0]
        runner = srt[:, 1] if self.B > 1 else np.full(hi - lo, np.inf)
        with np.errstate(invalid="ignore"):
            near = np.isfinite(best) & (runner - best <= TIE_TOL)
        self.compared += hi - lo
        self.left_out += int(near.sum())
        bad = np.flatnonzero((gl != wl) & ~near)
        assert bad.size == 0, (f"{tag}: position {lo + bad[0]} labelled bin {gl[bad[0]]}, oracle bin {wl[bad[0]]} "
                               f"(oracle distances {alld[bad[0]]}); {bad.size} of {hi - lo} positions differ")
        for i in np.flatnonzero(near):       # left out, yet the label must be one of the tied bins
            assert gl[i] >= 0 and alld[i, gl[i]] <= best[i] + TIE_TOL, \
                f"{tag}: position {lo + i} labelled bin {gl[i]}, oracle distances {alld[i]}"
        if self.empty_bin is not None and not np.any(want["lab_prev"] == self.empty_bin):
            assert np.all(np.isposinf(alld[:, self.empty_bin])) and not np.any(gl == self.empty_bin), \
                f"{tag}: a position was labelled with the empty bin {self.empty_bin}"


def _run_case(name, dev, check_counters=True, slice_names=("full", "inner", "one", "empty")):
    (N, D, B, m), seed, _env, metric, counters, exact_guess = CASES[name]
    X, initial, is_seed = _case_data(name)
    dev.set_samples(X)
    compared = left_out = rounds = 0
    for slice_name in slice_names:
        ref = OracleBackend(metric=metric, want_all=True, threads=ORACLE_THREADS)
        ref.set_samples(X)
        ref.fit_begin(B, initial, m)
        dev.fit_begin(B, initial, m)
        if check_counters:
            for cname, value in counters.items():
                assert dev.counter(cname) == value, (name, cname, dev.counter(cname))
        cmp = _Compare(ref, B, exact_guess)
        rng = np.random.default_rng(seed * 7 + 1)               # (the same batches and rounds for every slice shape)
        for bi, sl in enumerate(S.draw_batches(is_seed, rng)):
            K = len(sl)
            lo, hi = S.slices(K)[slice_name]
            cmp.empty_bin = B - 1 if (name == "small_bins" and bi == 0) else None
            S.run_batch([ref, dev], sl, lo, hi, B, rng, compare=cmp,
                        tag=f"{name}/{slice_name} [{lo}, {hi}) batch {bi} (K = {K})")
        assert np.array_equal(dev.fit_labels(), ref.fit_labels()), f"{name}/{slice_name}: labels after the commits"
        if check_counters:
            assert dev.counter("shortlist_short") == 0
            if name == "pools":
                print(f"{name}/{slice_name}: pool_batches = {dev.counter('pool_batches')}")
        compared += cmp.compared
        left_out += cmp.left_out
        rounds += cmp.rounds
    share = left_out / max(compared, 1)
    print(f"stepwise {name}: {rounds} rounds, {compared} positions compared, {left_out} left out of the label "
          f"comparison as near-ties ({share:.3%})")
    assert compared > 0 and share <= MAX_LEFT_OUT, (name, left_out, compared)
    return share


@pytest.mark.parametrize("name", list(CASES))
def test_every_round_equals_the_oracle(ctx, name):
    """Three batches (K = 96, 257, 40) per fit, one fit per slice shape, every round of the script against the oracle.
    `pools`: the stepwise entry points never run the threshold pools -- chb_fit_cluster's loop alone builds and keeps
    them -- so the case runs the ordinary two-sweep shortlist launch under the pool switches and shows no pool counter.
    `small_bins`: while a bin has no member and no entry of lab_prev names it, no position may be labelled with it."""
    env, metric = CASES[name][2], CASES[name][3]
    dev = _ctx_env(env) if env else ctx
    try:
        dev.set_metric(metric)
        _run_case(name, dev)
    finally:
        dev.set_metric("convex")
        if env:
            dev.close()


def test_all_hulls_empty(ctx):
    """No labelled sample at all: round 0 sees only empty hulls and must give -1 / +inf for every position (the
    comparison with the oracle checks exactly that); the later rounds see the batch's own entries as the only members."""
    X, _, _ = _case_data("small_bins")
    N, B, m = len(X), 6, 5
    initial = np.full(N, -1, dtype=np.int64)
    ref = OracleBackend(want_all=True)
    ref.set_samples(X)
    ref.fit_begin(B, initial, m)
    ctx.set_samples(X)
    ctx.fit_begin(B, initial, m)
    cmp = _Compare(ref, B, False)
    seen = []

    def compare(want, got):
        cmp(want, got)
        if got["kind"] == "guess":
            assert np.all(got["guess"] == -1)
        elif " round 0 " in got["tag"]:
            assert np.all(got["lab_new"] == -1) and np.all(np.isposinf(got["min_dist"]))
            seen.append(1)
    rng = np.random.default_rng(3)
    sl = rng.choice(N, size=40, replace=False)
    S.run_batch([ref, ctx], sl, 0, 40, B, rng, compare=compare, tag="no seeds")
    assert seen and np.array_equal(ctx.fit_labels(), ref.fit_labels())


def test_call_sequence_and_argument_errors(ctx):
    """Host-only refusals: none of these calls reaches a kernel.  After them the open batch still runs a valid round
    and commit, equal to the oracle's."""
    from chbin_amd._lib import ChbError
    (N, D, B, m) = CASES["fused5"][0]
    X, initial, is_seed = _case_data("fused5")
    ctx.set_samples(X)
    ctx.fit_begin(B, initial, m)
    K = 40
    sl = S.draw_batches(is_seed, np.random.default_rng(1), sizes=(K,))[0]
    lab = np.zeros(K, dtype=np.int64)
    out = np.full(K, S.LAB_SENTINEL, dtype=np.int64)
    md = np.full(K, S.DIST_SENTINEL)
    # ---- no open batch
    with pytest.raises(ChbError, match=r"error -4: no open batch"):
        ctx.batch_round(lab, 0, out, md)
    with pytest.raises(ChbError, match=r"error -4: no open batch"):
        ctx.batch_guess(out)
    with pytest.raises(ChbError, match=r"error -4: no open batch"):
        ctx.batch_commit(lab)
    # ---- bad perm_slice / slice geometry (the batch is not opened)
    dup = sl.copy()
    dup[7] = dup[3]
    with pytest.raises(ChbError, match=r"error -1: a batch lists a sample twice"):
        ctx.batch_begin(dup, 0, K)
    for v in (-1, N, 1 << 40):
        bad = sl.copy()
        bad[5] = v
        with pytest.raises(ChbError, match=r"error -1: perm entry out of range"):
            ctx.batch_begin(bad, 0, K)
    for lo, hi in ((-1, K), (0, K + 1), (9, 8)):
        with pytest.raises(ChbError, match=r"error -1: bad batch geometry"):
            ctx.batch_begin(sl, lo, hi)
    with pytest.raises(ChbError, match=r"error -1: bad batch geometry"):
        ctx.batch_begin(np.zeros(0, dtype=np.int64), 0, 0)
    with pytest.raises(ChbError, match=r"error -4: no open batch"):
        ctx.batch_commit(lab)
    # ---- an open batch, opened twice
    ref = OracleBackend()
    ref.set_samples(X)
    ref.fit_begin(B, initial, m)
    ref.batch_begin(sl, 0, K)
    ctx.batch_begin(sl, 0, K)
    with pytest.raises(ChbError, match=r"error -4: previous batch not committed"):
        ctx.batch_begin(sl, 0, K)
    # ---- labels outside [-1, B): lab_prev of a round, final_labels of a commit (2^32 would narrow to bin 0)
    lab_prev = ref.lab_old.copy()
    lab_prev[lab_prev < 0] = 1
    for pos, v in ((3, B), (K - 1, -2), (0, 1 << 32), (11, -(1 << 32) - 1)):
        bad = lab_prev.copy()
        bad[pos] = v
        with pytest.raises(ChbError, match=rf"error -1: lab_prev\[{pos}\] = {v} is outside \[-1, num_clusters\)"):
            ctx.batch_round(bad, 0, out, md)
        with pytest.raises(ChbError, match=rf"error -1: final_labels\[{pos}\] = {v} is outside \[-1, num_clusters\)"):
            ctx.batch_commit(bad)
    # ---- active outside [0, K], or smaller than the previous round's
    for a in (-1, K + 1):
        with pytest.raises(ChbError, match=r"error -1: active must be in \[0, K\]"):
            ctx.batch_round(lab_prev, a, out, md)
    assert np.all(out == S.LAB_SENTINEL) and np.all(md == S.DIST_SENTINEL)      # nothing was written by a refused call
    want, want_md = out.copy(), md.copy()
    ref.batch_round(lab_prev, 5, want, want_md)
    ctx.batch_round(lab_prev, 5, out, md)
    assert np.array_equal(out, want) and np.allclose(md[5:], want_md[5:], rtol=0, atol=QP_TOL)
    with pytest.raises(ChbError, match=r"error -1: active must not decrease within a batch"):
        ctx.batch_round(lab_prev, 4, out, md)
    # ---- the batch is intact: one more valid round and the commit
    lab_prev[5:] = want[5:]
    out[:], md[:], want[:], want_md[:] = S.LAB_SENTINEL, S.DIST_SENTINEL, S.LAB_SENTINEL, S.DIST_SENTINEL
    ref.batch_round(lab_prev, 5, want, want_md)
    ctx.batch_round(lab_prev, 5, out, md)
    assert np.array_equal(out, want) and np.allclose(md[5:], want_md[5:], rtol=0, atol=QP_TOL)
    lab_prev[5:] = want[5:]
    ref.batch_commit(lab_prev)
    ctx.batch_commit(lab_prev)
    assert np.array_equal(ctx.fit_labels(), ref.fit_labels())
    # a new batch starts at active 0 again
    ctx.batch_begin(sl, 0, K)
    ctx.batch_round(lab_prev, 0, out, md)
    ctx.batch_commit(lab_prev)


@pytest.mark.parametrize("N,D", [(300, 7), (257, 136), (200, 160), (150, 300)])
def test_set_samples_device_copies(ctx, O, N, D):
    """chb_set_samples_device copies: the caller's buffer is zeroed after the call, and the distances, a neighbour
    selection and a small fit are those of the same matrix uploaded from the host."""
    import chbin_amd
    from chbin_amd._lib import ChbError
    B, m = 3, 5
    X, initial, _ = chbin_amd.synth.make_synthetic(N, D, B, seed=N + D, sigma=8e-3, mix=0.5, n_seed=6)
    perms = chbin_amd.synth.draw_permutations(initial, 2, seed=0)
    t = torch.from_numpy(X).to("cuda")
    torch.cuda.synchronize()
    with pytest.raises(ChbError, match=r"error -1: "):
        ctx.set_samples_device(0, N, D)
    with pytest.raises(ChbError, match=r"error -1: "):
        ctx.set_samples_device(t.data_ptr(), 0, D)
    ctx.set_samples_device(t.data_ptr(), N, D)
    t.zero_()
    torch.cuda.synchronize()
    assert np.array_equal(ctx.pairwise_distance(), O.cdist(X))
    queries = np.arange(0, N, 7)
    labels = np.where(initial >= 0, initial, np.arange(N) % B)
    nb = ctx.topm_per_bin(labels, B, m, queries)
    fit = ctx.fit_cluster(B, initial, perms, m, 2, batch=64, want_min_dist=True)
    ctx.set_samples(X)
    nb_host = ctx.topm_per_bin(labels, B, m, queries)
    fit_host = ctx.fit_cluster(B, initial, perms, m, 2, batch=64, want_min_dist=True)
    for a, b in zip(nb, nb_host):
        assert np.array_equal(a, b)
    assert np.array_equal(fit[0], fit_host[0]) and fit[1] == fit_host[1] and np.array_equal(fit[2], fit_host[2])
    movable = initial < 0
    # (winning distances: a second fit over the same samples may run another formulation of the same kernels -- the
    #  context remembers what the first one found about tile skipping -- so they agree to the project's bound, not bitwise)
    assert np.all(np.isfinite(fit[3][movable]))
    assert np.abs(fit[3][movable] - fit_host[3][movable]).max() <= QP_TOL
    assert (fit[0][movable] >= 0).all()
