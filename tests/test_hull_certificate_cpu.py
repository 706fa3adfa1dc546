"""hull_certificate.py and the cases of wide_scale_cases.py, checked without a GPU: what test_gpu_wide_m_scales.py asks of
the wide kernels is satisfiable, by the reference alone.

  (a) on EVERY problem of every case the bracket [lo, hi] is narrower than 1e-10 of the scale -- the gap limit
      test_wide_m_cpu.py asserts for the oracle, not a new number -- with feasible weights behind it;
  (b) the bracket contains the suite's other yardsticks where they apply: oracle.enum_hull_distance up to 12 vertices
      and row_reference on wide_m_cases.wide(72) at m = 17 within row_reference.bound, the closed form at D = 1, the
      oracle's affine distance on independent sets;
  (c) the tie rule of test_gpu_row_scoring_scales.py (a row's bin goes unchecked when its reference margin is within twice
      the bound of its two best entries) leaves out at most 1 % of a case's rows; `identical`, `onehot` and the widths 1
      and 2, where ties are the construction, are exempt as there, and what they were built for is checked instead."""
import numpy as np
import pytest

import hull_certificate as H
import row_reference
import wide_m_cases as W
import wide_scale_cases as C

GAP = 1e-10   # of the scale (test_wide_m_cpu._envelope's limit)


def _width_and_ties(what, cert, exempt):
    fin = np.isfinite(cert.hi)
    assert np.array_equal(fin, np.isfinite(cert.lo)) and not np.isnan(cert.lo).any() and not np.isnan(cert.hi).any()
    assert np.all(cert.lo[fin] <= cert.hi[fin]) and np.all(cert.lo[fin] >= 0.0)
    assert np.all((cert.scale > 0.0) | ~fin | ((cert.lo == 0.0) & (cert.hi == 0.0)))   # scale 0: [0, 0]
    assert np.all(cert.hi[fin] <= cert.scale[fin] * (1.0 + 1e-15))   # (no hull point is farther than the farthest vertex)
    pos = fin & (cert.scale > 0.0)
    width = ((cert.hi[pos] - cert.lo[pos]) / cert.scale[pos]).max() if pos.any() else 0.0
    _, clear = row_reference.clear_rows(H.as_reference(cert))
    n_out = int(np.count_nonzero(~clear))
    print(f"{what}: largest (hi - lo) / scale = {width:.2e} over {int(pos.sum())} problems, "
          f"{n_out} of {len(clear)} rows within twice the bound of a tie")
    assert width <= GAP, (what, width)
    if not exempt:
        assert n_out <= 0.01 * len(clear), (what, n_out)


@pytest.mark.parametrize("kind", C.KINDS)
def test_scale_cases_close_their_brackets(kind):
    X, labels, Y, rows, _ = C.case_data(kind)
    sizes = np.bincount(labels[labels >= 0], minlength=C.B)
    assert sizes[C.SMALL] == C.N_SMALL and np.all(np.delete(sizes, C.SMALL) >= 64 + 1)   # full lists at m = 64
    assert X.shape == (C.N, C.dim(kind)) and Y.shape == (C.Q, C.dim(kind))
    assert np.all(np.isin(np.flatnonzero(labels == C.SMALL), rows)) and np.all(np.isin(np.arange(0, C.N, 6), rows))
    for m in C.MS:
        for call in ("recruit", "audit"):
            cert = C.case_certificate(kind, call, m)
            _width_and_ties(f"{kind} m={m} {call}", cert, kind in C.EXEMPT)
            assert np.isfinite(cert.hi).all()   # (no bin of these cases is empty)
            lens = np.array([[len(s) for s in per_bin] for per_bin in cert.sets])
            assert lens.max() == m and lens[:, C.SMALL].max() == min(m, C.N_SMALL) and lens.min() >= min(m, C.N_SMALL - 1)


@pytest.mark.parametrize("D", C.WIDTHS)
def test_width_cases_close_their_brackets(D):
    X, lab, Y, rows = C.width_data(D)
    assert tuple(np.bincount(lab, minlength=C.B)) == C.WSIZES and X.shape == (C.WN, D) and Y.shape == (C.WQ, D)
    for m in C.WMS:
        for call in ("recruit", "audit"):
            cert = C.width_certificate(D, call, m)
            _width_and_ties(f"D={D} m={m} {call}", cert, D in C.WEXEMPT)
            assert np.all(cert.hi[:, 0] == np.inf) and np.isfinite(cert.hi[:, 1:]).all()   # the bin without a member
            if D == 1:
                src = Y if call == "recruit" else X[rows]
                for q in range(len(src)):
                    for c in range(1, C.B):
                        want = C.closed_form_1d(src[q, 0], X[cert.sets[q][c], 0])
                        assert cert.lo[q, c] <= want <= cert.hi[q, c], (m, call, q, c)


@pytest.mark.parametrize("kind", C.KINDS)
def test_bracket_contains_the_enumerator(kind):
    """Up to 12 vertices the exhaustive enumerator is the suite's yardstick: on the leading 5 and 12 entries of the cases'
    own lists it lies in the bracket, within row_reference.bound."""
    from oracle import oracle as O
    X, labels, Y, _, _ = C.case_data(kind)
    rows = np.arange(0, C.Q, 5)
    sets = [C.case_sets(kind, "recruit")[q] for q in rows]
    zero = np.zeros(X.shape[1])
    for m in (5, 12):
        cert = H.certified_rows(X, labels, C.B, m, Y=Y, rows=rows, sets=sets)
        want = np.array([[O.enum_hull_distance(zero, np.ascontiguousarray(X[s[:m]] - Y[q])) for s in sets[k]]
                         for k, q in enumerate(rows)])
        bnd = row_reference.bound(row_reference.RowReference(want, cert.scale, None))
        pos = cert.scale > 0.0
        off = np.maximum(cert.lo - want, want - cert.hi)
        print(f"{kind} m={m}: enumerator outside the bracket by at most {(off[pos] / cert.scale[pos]).max():.2e} of the scale, "
              f"bracket width at most {((cert.hi - cert.lo)[pos] / cert.scale[pos]).max():.2e}")
        assert np.all(off <= bnd), (kind, m)
        assert np.all(want[~pos] == 0.0)


def test_bracket_contains_row_reference_on_friendly_data():
    rows, ref = W.audit_reference(72, 17, 40, every_seventh=True)
    X, lab, _, _ = W.wide(72, twins=40)
    cert = H.certified_rows(X, lab, W.B, 17, rows=rows)
    for q in range(len(rows)):
        for c in range(W.B):
            assert np.array_equal(cert.sets[q][c], ref.sets[q][c])
    fin = np.isfinite(ref.dist)
    assert np.array_equal(np.isfinite(cert.hi), fin) and np.array_equal(cert.scale, ref.scale)
    _width_and_ties("wide(72) m=17 audit", cert, False)
    with np.errstate(invalid="ignore"):   # (+inf against +inf in the bin without a member)
        off = np.maximum(cert.lo - ref.dist, ref.dist - cert.hi)[fin]
    print(f"wide(72) m=17: row_reference outside the bracket by at most {(off / ref.scale[fin]).max():.2e} of the scale")
    assert np.all(off <= row_reference.bound(ref)[fin])


def test_constructed_ties():
    """`identical`: a copy's m = 64 list holds equal entries only (the lowest 64 of the 150 equal members, the audited row
    withheld), spread over three member tiles and more, and its bracket is [0, 0].  `onehot`: nothing but exact ties; a
    bracket is [0, 0] or around sqrt(1 + 1 / n), n = 1 or 2 distinct points selected."""
    from oracle import oracle as O
    X, labels, Y, rows, copies = C.case_data("identical")
    equal = np.flatnonzero((X == Y[copies[0][0]]).all(axis=1) & (labels == 0))
    assert len(equal) >= 150 and len(copies[0]) >= 10 and len(copies[1]) >= 10
    members = np.flatnonzero(labels == 0)
    assert len(np.unique(np.searchsorted(members, equal) // 64)) >= 3
    for call, mine in (("recruit", copies[0]), ("audit", copies[1])):
        for m in C.MS:
            cert = C.case_certificate("identical", call, m)
            assert np.all(cert.lo[mine, 0] == 0.0) and np.all(cert.hi[mine, 0] == 0.0) and np.all(cert.scale[mine, 0] == 0.0)
            for q in mine:
                assert np.array_equal(cert.sets[q][0], equal[equal != (rows[q] if call == "audit" else -1)][:m])
    X, labels, Y, rows, _ = C.case_data("onehot")
    d = O.cdist_row(np.vstack([X, Y]), len(X) + 3)
    assert set(np.unique(d).tolist()) == {0.0, np.sqrt(2.0)}
    for call in ("recruit", "audit"):
        for m in C.MS:
            cert = C.case_certificate("onehot", call, m)
            zero = cert.hi == 0.0
            assert zero.any() and np.all(cert.lo[zero] == 0.0)
            near = np.abs(cert.hi[~zero][:, None] - np.sqrt(1.0 + 1.0 / np.array([1.0, 2.0]))[None, :]).min(axis=1)
            assert (~zero).any() and np.all(near < 1e-12)


def test_min_norm_point_on_known_problems():
    rng = np.random.default_rng(3)
    # a segment, a triangle that holds the origin, two thirds exact duplicates, one vertex on the origin
    seg = np.array([[1.0, -1.0], [1.0, 3.0]])
    tri = np.array([[-1.0, -1.0], [2.0, -1.0], [-1.0, 2.0]])
    for P, want in ((seg, 1.0), (tri, 0.0), (np.repeat(seg, 20, axis=0), 1.0), (np.vstack([tri + 5.0, np.zeros((1, 2))]), 0.0)):
        for s in (1.0, 1e-50, 1e+50):
            a = H.min_norm_point(s * P)
            assert a.shape == (len(P),) and np.all(a >= 0.0) and abs(a.sum() - 1.0) <= 1e-14
            lo, hi, scale = H.bracket(s * P, a)
            assert lo <= want * s <= hi and hi - lo <= 1e-14 * scale
    # duplicated random vertices in few dimensions, scaled columns
    for D, m in ((3, 17), (5, 33), (24, 64)):
        base = rng.normal(size=(m // 3 + 1, D)) * rng.lognormal(0, 3, size=(1, D)) + 1.0
        P = base[rng.integers(0, len(base), m)]
        a = H.min_norm_point(P)
        assert np.all(a >= 0.0) and abs(a.sum() - 1.0) <= 1e-14
        lo, hi, scale = H.bracket(P, a)
        assert hi - lo <= GAP * scale
        # any feasible weights give a valid bracket, only a wider one
        lo2, hi2, _ = H.bracket(P, np.full(m, 1.0 / m))
        assert lo2 <= hi and lo <= hi2 and hi2 - lo2 > hi - lo


def test_affine_distance_matches_the_oracle():
    from oracle import oracle as O
    X, labels, Y, _, _ = C.case_data("offset")
    sets = C.case_sets("offset", "recruit")
    zero = np.zeros(X.shape[1])
    worst = 0.0
    for q in range(0, C.Q, 13):
        for c in range(C.B):
            for m in (17, 64):
                P = np.ascontiguousarray(X[sets[q][c][:m]] - Y[q])
                scale = np.sqrt((P * P).sum(axis=1)).max()
                got, want = H.affine_distance(P), O.affine_hull_distance(zero, P)
                worst = max(worst, abs(got - want) / scale)
                assert got <= H.bracket(P, H.min_norm_point(P))[1]   # the affine hull contains the hull
    print(f"affine_distance against the oracle: at most {worst:.2e} of the scale")
    assert worst <= 1e-9
