"""The m <= 5 fused kernel's exchanges inside a 16-lane group (hull_solve16.h: row_xor_*, row_bcast_*; qp_kernels.hip:
reduce_scatter16, the work records of a pass) -- in-register DPP moves and LDS broadcasts where there were shuffles.

  test_helpers_equal_the_shuffles   the counter "lane_exchange_mismatches": one 256-thread launch compares every helper, on
                                    ints and on doubles (NaN payloads, -0.0, denormals, infinities), and the reduce-scatter
                                    built on them, bit for bit with the shuffle forms.  It also settles which way the two
                                    bank-masked moves of the xor-4 exchange shift.
  test_fit                          whole fits through the product library against the oracle: labels, sweeps and change
                                    counts equal, the winning distance of every movable row within QP_TOL = 1e-9, margins
                                    within 2e-9, seeds NaN (fit_replay.check_product).

Shapes of the fits, N = 3000, three seeds per bin, three sweeps at most:

  D      21 / 32 / 136 / 150   a row sweep's tail loop only / its main loop only / both / shadow rows of 160 columns (trim)
  B      9 / 24                unstriped / striped over the XCD lists with three bins each
  m      1 / 3 / 5
  batch  64 / 1024             with three members per bin at the start, the early batches hold pairs of 6, 7, 8..16 and more
                               than 16 candidates: the one-sweep classes, the wide passes, the trim and the exact path; the
                               batch-1024 fits must have trimmed pairs (fused_trim_pairs > 0)

The oracle replay of a (D, B, m) is computed once, on a thread pool, and shared by the two batch sizes: a fit's result does
not depend on the batch.

Seen on an MI355X: 0 mismatches; all 48 fits pass, the largest error of a winning distance is 5.6e-17, the batch-1024 fits
trim between 136 and 21,584 pairs, 12 s for the module."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fit_replay as R

pytestmark = pytest.mark.gpu

COUNTERS = R.COUNTERS + ["fused_trim_pairs", "fused_trim_in", "fused_trim_kept", "slow_pairs_last_round"]
DIMS, BINS, MS, BATCHES = (21, 32, 136, 150), (9, 24), (1, 3, 5), (64, 1024)


def _case(D, B, m, batch):
    return dict(N=3000, D=D, B=B, m=m, its=3, batch=batch, gen=dict(sigma=6e-3, mix=0.5, n_seed=3),
                expect=[("fused_enabled", "==", 1), ("prefilter_enabled", "==", 1)]
                + ([("fused_trim_pairs", ">", 0)] if batch == 1024 else []))


CASES = {f"d{D}-b{B}-m{m}-batch{batch}": _case(D, B, m, batch) for D in DIMS for B in BINS for m in MS for batch in BATCHES}
NAMES = list(CASES)


def _data_key(c):
    return c["D"], c["B"], c["m"]


def replay(X, B, initial, perms, m, its):
    """fit_replay.oracle_replay up to the sweep the reference stops at (its first sweep without a change)."""
    r = R.oracle_replay(X, B, initial, perms, m, its)
    still = np.flatnonzero(r[2] == 0)
    return replay(X, B, initial, perms, m, int(still[0]) + 1) if len(still) and still[0] + 1 < len(r[2]) else r


@pytest.fixture(scope="module")
def data():
    """Each (D, B, m) data set with its oracle replay on up to 8 threads (the oracle is a ctypes library: each call drops the
    GIL) while the GPU fits go on."""
    out, sets = {}, {}
    pool = ThreadPoolExecutor(max_workers=8)
    for name in NAMES:
        c = CASES[name]
        key = _data_key(c)
        if key not in sets:
            X, initial, perms = R.case_data(c)
            sets[key] = dict(X=X, initial=initial, perms=perms,
                             oracle=pool.submit(replay, X, c["B"], initial, perms, c["m"], c["its"]))
        out[name] = sets[key]
    yield out
    pool.shutdown(wait=False, cancel_futures=True)


def test_helpers_equal_the_shuffles():
    from chbin_amd import _lib
    ctx = _lib.Context(0)
    try:
        assert ctx.counter("lane_exchange_mismatches") == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_fit(data, name):
    c, d = CASES[name], data[name]
    worst, cnt = R.check_product(name, c, d, d["oracle"].result(), counters=COUNTERS)
    print(f"\n{name}: worst error of a winning distance {worst:.3g}")
    R.check_counters(name, c, cnt)
