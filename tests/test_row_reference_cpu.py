"""row_reference.reference_rows, the shift-invariant yardstick of test_gpu_row_scoring_scales.py, checked without a GPU:

  (a) on the unmodified friendly cases of test_gpu_recruit.py and test_gpu_audit.py it agrees with the yardstick those
      tests use (oracle.sweep with all distances) within their QP_TOL, the +inf pattern exactly;
  (b) it is invariant: scaling the data by 2^-40 scales every distance bit for bit (a power of two is exact), adding
      1000 to every entry moves a distance by at most 1e-9 of its scale -- the old yardstick on the same shifted data is
      printed next to it, without an assertion, to show the size of its loss;
  (c) on every case of test_gpu_row_scoring_scales.py but the kinds whose ties are the construction, the rule that lets a
      row's bin go unchecked (reference margin within twice the bound of its two best entries) leaves out at most 1 % of
      the rows: the GPU test's cap, proven from the reference alone."""
import numpy as np
import pytest

import test_gpu_audit as A
import test_gpu_recruit as R
import test_gpu_row_scoring_scales as S
from row_reference import bound, reference_rows

QP_TOL = R.QP_TOL


def _agree(name, ref, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(ref.dist), fin), name
    assert np.array_equal(ref.dist[~fin], want[~fin]), name
    err = np.abs(ref.dist[fin] - want[fin]).max()
    print(f"{name}: largest |reference - oracle.sweep| = {err:.3e} over {int(fin.sum())} entries")
    assert err <= QP_TOL, (name, err)


@pytest.mark.parametrize("name", ["base", "m15"])
def test_agrees_with_the_recruit_oracle(name):
    c = R.CASES[name]
    X, labels, Y = R.case_data(name)
    ref = reference_rows(X, labels, c["B"], c["m"], Y=Y)
    assert ref.dist.shape == (c["Q"], c["B"]) and ref.dist.dtype == np.float64 and ref.sets is None
    _agree(name, ref, R.oracle_rows(X, labels, Y, c["B"], c["m"]))
    assert np.all(ref.scale[np.isfinite(ref.dist)] > 0.0)


def test_agrees_with_the_audit_oracle():
    c = A.CASES["base"]
    X, labels, rows = A.case_data("base")
    assert rows is None
    ref = reference_rows(X, labels, c["B"], c["m"])
    _agree("audit base", ref, A.oracle_rows(X, labels, np.arange(len(X)), c["B"], c["m"]))


def test_sets_and_leave_one_out():
    """The index sets are the oracle's selection; an audited row is never in its own set, a twin is."""
    from oracle import oracle as O
    c = A.CASES["m16_dups"]
    X, labels, _ = A.case_data("m16_dups")
    B, m = c["B"], c["m"]
    rows = np.arange(0, len(X), 7)
    ref = reference_rows(X, labels, B, m, rows=rows, want_sets=True)
    twins = 0
    for k, r in enumerate(rows):
        lab = labels.copy()
        lab[r] = -1
        row = O.cdist_row(X, int(r))
        for b in range(B):
            assert np.array_equal(ref.sets[k][b], O.find_nearest_from_cluster(b, lab, row, m))
            assert r not in ref.sets[k][b]
            if len(ref.sets[k][b]) and row[ref.sets[k][b][0]] == 0.0:
                twins += 1   # (13 to 16 vertices: Goldfarb-Idnani's zero is a rounding-sized number, the envelope's allowance)
                assert ref.dist[k, b] <= bound(ref)[k, b]
    assert twins > 10
    # a recruited row withholds nothing: a copy of a labelled sample is at distance 0 from its bin
    src = np.flatnonzero(labels >= 0)[:5]
    got = reference_rows(X, labels, B, m, Y=X[src], want_sets=True)
    for k, s in enumerate(src):
        assert s in got.sets[k][labels[s]] and got.dist[k, labels[s]] <= bound(got)[k, labels[s]]


@pytest.mark.parametrize("name", ["base", "m15"])
def test_invariance(name):
    c = R.CASES[name]
    B, m = c["B"], c["m"]
    X, labels, Y = R.case_data(name)
    rows = np.arange(0, c["Q"], 5)
    arows = np.arange(0, len(X), 11)
    plain = reference_rows(X, labels, B, m, Y=Y, rows=rows)
    aplain = reference_rows(X, labels, B, m, rows=arows)
    # a power of two: bit for bit
    s = 2.0 ** -40
    for got, want in ((reference_rows(s * X, labels, B, m, Y=s * Y, rows=rows), plain),
                      (reference_rows(s * X, labels, B, m, rows=arows), aplain)):
        assert np.array_equal(got.dist.view(np.uint64), (s * want.dist).view(np.uint64)), name
        assert np.array_equal(got.scale.view(np.uint64), (s * want.scale).view(np.uint64)), name
    # a common offset: within 1e-9 of the scale
    t = 1000.0
    for got, want, call in ((reference_rows(X + t, labels, B, m, Y=Y + t, rows=rows), plain, "recruit"),
                            (reference_rows(X + t, labels, B, m, rows=arows), aplain, "audit")):
        assert np.array_equal(np.isfinite(got.dist), np.isfinite(want.dist))
        fin = np.isfinite(want.dist)
        rel = (np.abs(got.dist - want.dist)[fin] / want.scale[fin]).max()
        print(f"{name} {call}: reference(X + {t:g}) against reference(X): worst {rel:.3e} of the scale")
        assert np.all(np.abs(got.dist - want.dist)[fin] <= 1e-9 * want.scale[fin]), (name, call, rel)
    # the old yardstick on the shifted data (no assertion: this is the loss the new reference is there to avoid)
    old = R.oracle_rows(X + t, labels, Y + t, B, m, rows=list(rows))
    fin = np.isfinite(plain.dist)
    loss = np.abs(old - plain.dist)[fin]
    print(f"{name}: oracle.sweep on X + {t:g} against reference(X): worst {loss.max():.3e} absolute, "
          f"{(loss / plain.scale[fin]).max():.3e} of the scale")


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n]["kind"] not in S.EXEMPT])
def test_tie_rule_leaves_out_at_most_one_percent(name):
    for call in ("recruit", "audit"):
        n_out, n = S.left_out(name, call)
        print(f"{name} {call}: {n_out} of {n} rows within twice the bound of a tie")
        assert n_out <= 0.01 * n, (name, call, n_out, n)


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n]["kind"] in S.EXEMPT])
def test_constructed_ties(name):
    """The two exempt kinds do what they were made for: `identical` puts copies of 150 equal members of bin 0 among the
    scored rows (reference distance exactly 0, the whole selected set equal to the row at the case's m), `onehot` knows
    no distance but 0 and sqrt(2)."""
    from oracle import oracle as O
    c = S.CASES[name]
    X, labels, Y, rows, copies = S.case_data(name)
    if c["kind"] == "identical":
        equal = np.flatnonzero((X == Y[copies[0][0]]).all(axis=1) & (labels == 0))
        assert len(equal) >= S.N_EQUAL > 2 * 64 and S.N_EQUAL > c["m"]
        members = np.flatnonzero(labels == 0)
        assert len(np.unique(np.searchsorted(members, equal) // 64)) >= 3   # (spread over three member tiles and more)
        for call, mine in (("recruit", copies[0]), ("audit", copies[1])):
            ref = S.case_reference(name, call)
            assert len(mine) >= S.N_COPIES
            assert np.all(ref.dist[mine, 0] == 0.0) and np.all(ref.scale[mine, 0] == 0.0)
            for q in mine:
                assert np.array_equal(ref.sets[q][0], equal[equal != (rows[q] if call == "audit" else -1)][:c["m"]])
    else:
        d = O.cdist_row(np.vstack([X, Y]), len(X) + 3)
        assert set(np.unique(d).tolist()) == {0.0, np.sqrt(2.0)}
