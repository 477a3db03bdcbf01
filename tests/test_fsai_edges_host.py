"""The FSAI edge cases (tests/fsai_edge_cases.py) on the CPU: the width facts the GPU tests rely on, the numpy restatement
(tests/fsai_restatement.py) against a reference that does not share its operation order, and what it refuses.

THE REFERENCE.  For column i with B = A[P_i, P_i] (the full symmetric block, gathered entry by entry from A's lower triangle -- the
only part the contract reads; S A S of `scaled_rows` is symmetric up to rounding only -- not through the restatement's index
arithmetic) and l the restated column, g = B l is formed in np.longdouble.  FSAI is defined by g_p = 0 (p > 0)
and g_0 l_0 = 1, so the residuals

    rho_p = |g_p| / (u (|B| |l|)_p)   (p > 0),        rho_0 = |g_0 l_0 - 1| / (u (|B| |l|)_0 |l_0|)         (u = 2^-53)

are invariant under a diagonal scaling of A up to rounding and must stay below a constant c.  MEASURED worst rho per case (x86-64
glibc, numpy 2.x; `pytest -s` prints them again):

    banded200_63 11.55   banded150_21_l3 6.84   banded200_63_scaled8 10.60   banded200_63_scaled70 10.87   random_bbt600 5.02
    stored_zeros_poisson20 2.71   jumping24_b4 2.95   anisotropic24 1.93   tiny_components 2.84   boundary_identity20 1.82
    tiny1 1.05   tiny2 4.08   tiny3 4.08   diags130 3.73   poisson16_band40_pattern 3.24

(worst residual over the a-priori limit below: 0.67, random_bbt600).  The test allows 4 x the measured value of each case
(head-room for another libm or scaling seed).  The a-priori limit holds too: a Cholesky solve has (B + dB) y = e_1 with |dB| <= gamma_{3m+1} |C| |C^T| (Higham, Accuracy and Stability, theorem 10.4) and the
scaling by 1 / sqrt(y_0) adds two roundings, so |residual_p| <= gamma_{3m+3} (|C| |C^T| |l|)_p with C the (fp64, LAPACK) Cholesky
factor of B -- asserted for every column as the upper sanity limit.
"""

import numpy as np
import pytest
import scipy.sparse as sp

import fsai_edge_cases as X
import fsai_restatement as R

U = 2.0 ** -53
HEADROOM = 4.0
# the worst rho of each case as measured (the docstring); the bound of the test is HEADROOM x this
MEASURED_RHO = {
    "banded200_63": 11.55, "banded150_21_l3": 6.84, "banded200_63_scaled8": 10.60, "banded200_63_scaled70": 10.87,
    "random_bbt600": 5.02, "stored_zeros_poisson20": 2.71, "jumping24_b4": 2.95, "anisotropic24": 1.93, "tiny_components": 2.84,
    "boundary_identity20": 1.82, "tiny1": 1.05, "tiny2": 4.08, "tiny3": 4.08, "diags130": 3.73, "poisson16_band40_pattern": 3.24,
}


def _pattern(case):
    return case.pattern() if case.pattern is not None else None


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_width_facts(case):
    A = case.matrix()
    assert A.has_sorted_indices and A.shape[0] <= 2000
    counts, max_m = R.width_class_counts(A, level=case.level, pattern=_pattern(case))
    assert tuple(counts) == case.counts and max_m == case.max_m and sum(counts) == A.shape[0]
    up, _ = R.upper_pattern(A, case.level, _pattern(case))
    m = np.diff(up)
    for width, count in case.hits.items():
        assert int(np.count_nonzero(m == width)) == count, f"width {width}"
    assert set(range(1, case.all_widths_to + 1)) <= set(m.tolist())


def test_table_reaches_every_class_and_boundary():
    """Over the table: every class holds columns, some case leaves each of the four upper classes empty, one class holds exactly one
    column, and both sides of every boundary (4|5, 8|9, 16|17, 32|33) and the cap occur."""
    total = np.sum([c.counts for c in X.CASES], axis=0)
    assert (total > 0).all()
    for k in range(1, 5):
        assert any(c.counts[k] == 0 for c in X.CASES)
    assert any(1 in c.counts for c in X.CASES)
    assert all(w in X.CASE_BY_NAME["banded200_63"].hits for w in X.BOUNDARY_WIDTHS + (64,))
    A = X.CASE_BY_NAME["banded200_63_scaled70"].matrix()
    d = A.diagonal()
    assert d.min() < 1e-100 and d.max() > 1e100                     # sqrt, the pivot test and y / sqrt(y_0) see 1e+-100
    A = X.CASE_BY_NAME["random_bbt600"].matrix()
    off = A.data[A.indices != np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))]
    assert (off > 0).any() and (off < 0).any()
    A = X.CASE_BY_NAME["stored_zeros_poisson20"].matrix()
    assert np.count_nonzero(A.data == 0.0) > 100
    # the explicit pattern is much wider than A: most pairs of a local system are absent from A
    c = X.CASE_BY_NAME["poisson16_band40_pattern"]
    assert c.pattern().nnz > 10 * sp.tril(c.matrix()).nnz


def _worst_rho(A, up, ui, hv):
    """(worst rho, worst residual / (gamma_{3m+3} |C||C^T||l|)) over every column; B is gathered from A entry by entry."""
    Ad = {}
    Ac = A.tocoo()
    for r, c, v in zip(Ac.row.tolist(), Ac.col.tolist(), Ac.data.tolist()):
        Ad[(r, c)] = v
    worst, worst_apriori = 0.0, 0.0
    for i in range(A.shape[0]):
        P = ui[up[i]:up[i + 1]].tolist()
        m = len(P)
        assert P[0] == i
        B = np.array([[Ad.get((max(r, c), min(r, c)), 0.0) for c in P] for r in P])      # the lower triangle of A, mirrored
        l = hv[up[i]:up[i + 1]]
        Bl, ll = B.astype(np.longdouble), l.astype(np.longdouble)
        g = Bl @ ll
        res = np.abs(g)
        res[0] = abs(g[0] * ll[0] - 1)
        scale = np.abs(Bl) @ np.abs(ll)
        scale[0] *= abs(ll[0])
        dead = scale == 0                        # (a component that only meets exact zeros: stored zeros, identity rows)
        assert (res[dead] == 0).all()
        scale[dead] = 1
        worst = max(worst, float((res / (U * scale)).max()))
        # the a-priori limit, scaled to a unit diagonal first so that LAPACK's Cholesky sees no over- or underflow
        s = 1.0 / np.sqrt(np.diag(B))
        C = np.linalg.cholesky(B * s[:, None] * s[None, :]).astype(np.longdouble) / s.astype(np.longdouble)[:, None]
        cc = (np.abs(C) @ np.abs(C.T)) @ np.abs(ll)
        cc[0] *= abs(ll[0])
        cc[dead] = 1
        k = 3 * m + 3
        worst_apriori = max(worst_apriori, float((res / (k * U / (1 - k * U) * cc)).max()))
    return worst, worst_apriori


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_restatement_against_long_double(case):
    A = case.matrix()
    up, ui, hv = R.fsai_upper(A, case.level, _pattern(case))
    assert np.isfinite(hv).all()
    rho, apriori = _worst_rho(A, up, ui, hv)
    print(f"{case.name}: worst rho {rho:.3f} (allowed {HEADROOM * MEASURED_RHO[case.name]:.2f}), "
          f"worst residual / a-priori limit {apriori:.4f}")
    assert rho <= HEADROOM * MEASURED_RHO[case.name]
    assert apriori <= 1.0
    # and L = the transpose of H: every column of L is the solve of its local system
    L = R.fsai(A, level=case.level, pattern=_pattern(case))
    H = sp.csr_matrix((hv, ui, up), shape=A.shape)
    assert (L.T.tocsr() != H).nnz == 0
    assert np.array_equal(L.indices[L.indptr[1:] - 1], np.arange(A.shape[0]))


@pytest.mark.parametrize("case", X.ERROR_CASES, ids=lambda c: c.name)
def test_restatement_refuses(case):
    A = case.matrix()
    with pytest.raises(R.FsaiError) as e:
        R.fsai(A, level=case.level)
    assert (e.value.kind, e.value.column) == (case.kind, case.column)
    if case.kind == "width":
        assert f"column {case.column} has m = {case.m} " in str(e.value)
    else:
        assert f"column {case.column}" in str(e.value)


def test_pivot_cases_fail_where_they_are_meant_to():
    """What makes each pivot case a case: two failing columns of which the lower one is named; a failing column in a register class
    below failing columns of a wide class; Cholesky pivots that all pass where only y_0 overflows."""
    def failing(A, level):
        up, ui = R.upper_pattern(A, level)
        bad = []
        for m in np.unique(np.diff(up)):
            cols = np.flatnonzero(np.diff(up) == m)
            B, _ = R.local_systems(A, cols, up, ui, int(m))
            bad += cols[R.solve_columns(B)[1]].tolist()
        return sorted(bad), np.diff(up)
    bad, m = failing(X.ERROR_CASE_BY_NAME["banded200_20_neg30_neg170"].matrix(), 1)
    assert bad == list(range(10, 31)) + list(range(150, 171))
    bad, m = failing(X.ERROR_CASE_BY_NAME["reg_and_wide_both_fail"].matrix(), 1)
    assert bad == [1, 2] + list(range(33, 54)) and m[1] == 2 and m[2] == 1 and (m[33:54] == 21).all()
    bad, m = failing(X.ERROR_CASE_BY_NAME["banded200_63_neg150"].matrix(), 1)
    assert bad[0] == 87 and m[87] == 64                              # the `bad` path of the 64-wide kernel
    for name, col in (("y0_overflows_reg", 5), ("y0_overflows_wide", 0)):
        c = X.ERROR_CASE_BY_NAME[name]
        A = c.matrix()
        up, ui = R.upper_pattern(A, c.level)
        P = ui[up[col]:up[col + 1]]
        B = A[P][:, P].toarray()
        with np.errstate(over="ignore"):
            C = np.linalg.cholesky(B * 2.0 ** 1000) * 2.0 ** -500   # (scaled out of the subnormal range for LAPACK)
            assert np.isfinite(C).all() and (np.diag(C) > 0).all() and not np.isfinite(1.0 / B[0, 0])


@pytest.mark.parametrize("disorder", [X.reversed_rows, X.first_two_swapped])
def test_unsorted_parts_are_the_same_matrix(disorder):
    for A in (X.E.poisson2d(24), X.E.random_bbt(300)):
        rp, ci, v = disorder(A)
        B = sp.csr_matrix((v, ci, rp), shape=A.shape)
        assert not B.has_sorted_indices and np.array_equal(rp, A.indptr)
        assert (B != A).nnz == 0
        assert all(i in ci[rp[i]:rp[i + 1]] for i in range(A.shape[0]))
