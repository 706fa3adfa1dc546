"""Whole fits at every num_neighbors (m) from 1 to 17, every hull distance checked against the oracle.

m decides which kernel serves a fit and which host rules apply; the other whole-fit modules stand on a handful of m.  Here
one case per (family, route, m) runs both halves of test_gpu_bin_distances.py (shared through fit_replay.py):

  (a) product library, in process: labels, sweeps and changes per sweep equal the oracle's, min_dist is the row minimum of
      the oracle's distances of the last sweep within QP_TOL, margin within 2 * QP_TOL, seeds NaN, shortlist_short == 0;
  (b) developer library, in a child (CHB_DEV_ALL_DIST, CHB_SL_BOUNDS=1, CHB_SL_VALIDATE=1): every one of the n_move x B
      distances of the last sweep within QP_TOL of the oracle's, +inf exactly where the oracle has it, the dumped rows'
      winner and runner-up what min_dist and margin report.

What m selects -- the map from a failing m to a kernel:

  boundary                     what changes there
  m <= 5 / 6..16               fused path: hull_select_qp_kernel<5, ...> / hull_select_qp16_kernel (launch_hull_select_qp,
                               qp_kernels.hip)
  m <= 4 / 5 / 6..8 / 9..16    list path (CHB_FUSED=0, or no shortlist stage): hull_qp_kernel<4> / <5> / <8> /
                               hull_qp16_kernel (dispatch, qp_kernels.hip)
  m <= 8 / 9..16               list path: rescore_kernel<8, 2> / rescore_kernel<16, 4> (launch_rescore, topm_kernels.hip)
  m <= 8 / m > 8               threshold pools are built at all (pool_build, chb_api.hip: m > 8 keeps the two-sweep
                               shortlist); the pool thresholds are the m-th nearest of a 32-row tile
  m + 3                        pool drop rule pc > (m + 3) * pp in the fit driver
  m <= 16 / m = 17             launch_topm + tuned kernels / launch_topm_generic + hull_generic_kernel (kMaxM)

Families (fit_replay.FAMILIES; data by the seed rule of fit_replay.case_data, permutations with seed 0):

  full    N = 500, D = 64, B = 4, 20 seeds per bin, two sweeps: every list is full from the first visit.  m = 1..17
  short   the same with 3 seeds per bin and ONE sweep: for m >= 4 every bin starts below m members and grows past m inside
          the compared sweep.  m = 1..17 (m = 4 on the next seed, see fit_replay.FAMILIES)
  stuck   short's m = 4 data by the seed rule: one bin keeps its three seeds, its list is short of m at every visit
  pools   shape and switches of test_gpu_bin_distances.py's pool_m5_batch257 (N = 2500, D = 136, B = 8, batch 257,
          CHB_POOL_TAU=2, CHB_TILE_SKIP=0): m = 1, 2, 3, 4, 6, 7, 8 must run with pools, m = 9 -- the other side of
          pool_build's rule -- without

Routes and the counters that prove them (a case whose counters contradict this fails; with m they determine the kernel):

  default  no switch       prefilter_enabled == 1; fused_enabled == 1 for m <= 16, == 0 for m = 17
  lists    CHB_FUSED=0     fused_enabled == 0, prefilter_enabled == 1              (m <= 16)
  pooled   the pool pair   pool_batches > 0 for m <= 8, == 0 for m = 9; fused_enabled == 1

test_fit_neighbors_cpu.py shows from the oracle alone that no visit of these fits is decided by less than 10 * QP_TOL, which
makes label equality a fair demand.  The oracle replays are computed once per (family, m) on a thread pool and shared by
the routes; the developer children run one per family and route, one after another, when their first case asks.

Seen on an MI355X: every case passes; the largest error of any distance is 5.6e-17 (pools, m = 1), per family and route
3.5e-17 / 4.2e-17 (full: default / lists), 4.2e-17 / 4.2e-17 (short), 2.8e-17 / 2.8e-17 (stuck).  The pooled fits keep their
pools through all 20 batches for m <= 4 and drop them by the (m + 3) rule after 11 / 8 / 7 pooled batches at m = 6 / 7 / 8."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fit_replay as R

pytestmark = pytest.mark.gpu

CASES = R.neighbor_cases()
NAMES = list(CASES)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """Each (family, m) data set (also written for the developer children) with its oracle replay on up to 8 threads (the
    oracle is a ctypes library: each call drops the GIL) while the GPU tests go on; the routes of a family share both."""
    tmp = tmp_path_factory.mktemp("fit_neighbors")
    out, sets = {"_tmp": tmp}, {}
    pool = ThreadPoolExecutor(max_workers=8)
    for name in NAMES:
        c = CASES[name]
        key = R.neighbor_data_name(c["family"], c["m"])
        if key not in sets:
            X, initial, perms = R.case_data(c)
            path = str(tmp / f"{key}.npz")
            np.savez(path, X=X, initial=initial, perms=perms)
            fut = pool.submit(R.oracle_replay, X, c["B"], initial, perms, c["m"], c["its"])
            sets[key] = dict(X=X, initial=initial, perms=perms, npz=path, oracle=fut)
        out[name] = sets[key]
    yield out
    pool.shutdown(wait=False, cancel_futures=True)


class _Children:
    """One developer child per (family, route), started when its first case asks and never a second time: a child that
    failed fails each of its cases with what it left."""

    def __init__(self, data):
        self.data, self.done = data, {}

    def get(self, name):
        c = CASES[name]
        key = (c["family"], c["route"])
        if key not in self.done:
            names = [n for n in NAMES if (CASES[n]["family"], CASES[n]["route"]) == key]
            # a child's serial work: the interpreter and the library (a few seconds), then per case a context and one fit
            # of at most 2500 rows with the shortlist checks on (well under a second each on an MI355X)
            try:
                self.done[key] = R.run_child(self.data, f"{key[0]}_{key[1]}", names, {}, CASES,
                                             timeout=60 + 10 * len(names))
            except (Exception, pytest.fail.Exception) as e:   # (a missing library and the timeout included)
                self.done[key] = e
        if isinstance(self.done[key], BaseException):
            raise AssertionError(f"developer child {key}: {self.done[key]!r}"[:6000])
        return self.done[key][name]


@pytest.fixture(scope="module")
def children(data):
    return _Children(data)


@pytest.mark.parametrize("name", NAMES)
def test_fit(data, children, name):
    c, d = CASES[name], data[name]
    oracle = d["oracle"].result()
    failures = []
    try:   # (a)
        worst_a, cnt = R.check_product(name, c, d, oracle)
        R.check_counters(name, c, cnt)
    except AssertionError as e:
        failures.append(("product", e))
    try:   # (b)
        rec, got, outs = children.get(name)
        worst_b = R.check_all_distances(name, c, d, oracle, rec, got, outs, "dev")
        print(f"\n[b] {name}: {int(np.isfinite(got).sum())} finite + {int(np.isinf(got).sum())} +inf distances, worst "
              f"error {worst_b:.3g} (min_dist of [a]: {worst_a if not failures else float('nan'):.3g}); "
              f"counters {rec['counters']}")
    except AssertionError as e:
        failures.append(("developer", e))
    if len(failures) == 1:
        raise failures[0][1]
    assert not failures, failures
