"""The data of test_gpu_fit_neighbors.py, judged by the oracle alone: is label equality a fair demand of those fits?

A fit's labels equal the oracle's only if no visit's winner is decided inside the solvers' tolerance.  For every (family, m)
of fit_replay.FAMILIES the oracle runs every sweep with all B hull distances of every visit (fit_replay.oracle_all_sweeps),
and

  * the smallest margin (second-smallest minus smallest finite distance) over every visit of EVERY sweep is at least
    10 * QP_TOL = 1e-8: a kernel within QP_TOL of the oracle on both distances cannot swap a winner;
  * `full`: every bin holds at least 17 members before the first visit (every list of every m <= 17 is full throughout);
  * `short`: for every m >= 4 every bin holds fewer than m members before the first visit and at least m after the sweep
    (the lists grow past m inside the one compared sweep).  m = 4 misses this with the seed of the rule (572: bin 2 wins no
    visit and keeps its three seeds), so it takes the next seed, 573; the 572 data stays as the family `stuck`, which must
    show just that -- a bin below m after the sweep, its list short at every visit;
  * no bin is empty at the start, so every compared distance is finite;
  * the last sweep of oracle_all_sweeps is what oracle_replay -- the GPU module's yardstick -- returns (checked for m <= 8,
    where a second replay costs little).

Smallest margins with the seed rule of fit_replay.case_data (N + D + B + m): `full` 3.9e-6 (m = 4), `short` 2.3e-6 (m = 11),
`stuck` 1.0e-6, `pools` 1.8e-8 (m = 7; next 5.7e-8 at m = 1).  If a change of the generator makes a case miss the limit, take
the next seed for that case and say so here; the limit stays."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fit_replay as R

MIN_MARGIN = 10 * R.QP_TOL
PAIRS = [(family, m) for family, f in R.FAMILIES.items() for m in f["ms"]]


def _judge(family, m):
    c = R.neighbor_data_case(family, m)
    X, initial, perms = R.case_data(c)
    sweeps = R.oracle_all_sweeps(X, c["B"], initial, perms, m, c["its"])
    mv = initial < 0
    margins = []
    for before, after, alld in sweeps:
        best, second = R.min2(alld[mv])
        assert np.all(np.isfinite(alld[mv])), (family, m)
        margins.append(float(np.min(second - best)))
    replay = R.oracle_replay(X, c["B"], initial, perms, m, c["its"]) if m <= 8 else None
    return dict(c=c, initial=initial, sweeps=sweeps, margins=margins, replay=replay)


@pytest.fixture(scope="module")
def judged():
    """Every (family, m) on a thread pool (the oracle is a ctypes library: each call drops the GIL), dearest first."""
    pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    order = sorted(PAIRS, key=lambda p: -R.FAMILIES[p[0]]["N"] * p[1])
    futs = {p: pool.submit(_judge, *p) for p in order}
    yield futs
    pool.shutdown(wait=False, cancel_futures=True)


@pytest.mark.parametrize("family,m", PAIRS)
def test_margins_and_bin_sizes(judged, family, m):
    j = judged[(family, m)].result()
    c, initial, sweeps = j["c"], j["initial"], j["sweeps"]
    B = c["B"]
    start = np.bincount(initial[initial >= 0], minlength=B)
    end = np.bincount(sweeps[-1][1][sweeps[-1][1] >= 0], minlength=B)
    print(f"\n{family} m={m}: smallest margin {min(j['margins']):.3g} (per sweep {['%.3g' % x for x in j['margins']]}), "
          f"bin sizes {start.tolist()} -> {end.tolist()}")
    assert len(sweeps) == c["its"], (family, m, "the oracle converged before the compared sweep")
    assert min(j["margins"]) >= MIN_MARGIN, (family, m, j["margins"])
    assert np.all(start > 0), (family, m, start)
    if family == "full":
        assert np.all(start >= 17), (family, m, start)
    if family == "short" and m >= 4:
        assert c["its"] == 1 and np.all(start < m) and np.all(end >= m), (family, m, start, end)
    if family == "stuck":
        assert c["its"] == 1 and "seed" not in c and np.all(start < m) and np.any(end < m), (family, m, start, end)
    if j["replay"] is not None:
        lab, its, ch, alld = j["replay"]
        assert its == len(sweeps) and np.array_equal(lab, sweeps[-1][1])
        assert np.array_equal(ch, [np.count_nonzero(a != b) for b, a, _ in sweeps])
        assert np.array_equal(alld, sweeps[-1][2], equal_nan=True)


def test_cases_cover_every_route_and_m():
    """The GPU module's ids: both routes of `full` and `short` at m = 1..17 / 1..16, `pools` at every m <= 9 but 5; each
    case's data set is one of PAIRS."""
    cases = R.neighbor_cases()
    want = [f"{f}-default-m{m}" for f in ("full", "short") for m in range(1, 18)]
    want += [f"{f}-lists-m{m}" for f in ("full", "short") for m in range(1, 17)]
    want += [f"pools-pooled-m{m}" for m in (1, 2, 3, 4, 6, 7, 8, 9)] + ["stuck-default-m4", "stuck-lists-m4"]
    assert sorted(cases) == sorted(want)
    for name, c in cases.items():
        assert (c["family"], c["m"]) in PAIRS, name
        d = R.neighbor_data_case(c["family"], c["m"])
        assert {k: c[k] for k in d} == d, name
