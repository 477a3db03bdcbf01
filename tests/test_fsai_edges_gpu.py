"""The device FSAI (dpcg_fsai.hip) at its edges, case table in tests/fsai_edge_cases.py (its width facts are asserted on the CPU by
tests/test_fsai_edges_host.py): the factor against the numpy restatement bit for bit on both sides of every width-class boundary,
at the cap m = 64, in padded and partly filled waves, on scaled, signed and zero-holding values; every refusal with the column the
restatement names; the cache's states after failures; unsorted input; the apply and a solve through 64-wide rows."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_matrices as E
import fsai_edge_cases as X
import fsai_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def restated():
    """The restated factor of a table case, computed once and never written to."""
    cache = {}

    def get(name):
        if name not in cache:
            c = X.CASE_BY_NAME[name]
            A = c.matrix()
            Lr = R.fsai(A, level=c.level, pattern=c.pattern() if c.pattern is not None else None)
            Lr.data.setflags(write=False)
            cache[name] = (A, Lr)
        return cache[name]
    return get


def _dev(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda()


def _factor(S):
    rp, ci, v = S.factor()
    return sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))


def _same_bits(X_, Y):
    return (np.array_equal(X_.indptr, Y.indptr) and np.array_equal(X_.indices, Y.indices)
            and np.array_equal(X_.data.view(np.uint64), Y.data.view(np.uint64)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _attach(D, S, case):
    S.set_preconditioner(D.FSAI(level=case.level) if case.pattern is None else D.FSAI(pattern=case.pattern()))


def _check_info(S, case):
    info = S.fsai_info()
    assert info["level"] == (case.level if case.pattern is None else 0) and info["max_m"] == case.max_m
    assert tuple(info["columns_by_width"][w] for w in R.WIDTH_CLASSES) == case.counts


# ---- factor bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_factor_equals_restatement(D, restated, case):
    A, Lr = restated(case.name)
    S = D.CsrSystem.from_any(A, reorder=None)
    _attach(D, S, case)
    _check_info(S, case)
    assert not S.fsai_info()["pattern_reused"]
    assert S.info()["precond"] == D._lib.PRECOND_LLT_MULTIPLY and S.info()["precond_nnz"] == Lr.nnz
    assert _same_bits(_factor(S), Lr)
    S.close()


@pytest.mark.parametrize("name", ["banded200_63", "banded200_63_scaled70"])
def test_reordered_handle_gives_the_caller_s_numbering(D, restated, name):
    A, Lr = restated(name)
    S = D.CsrSystem.from_any(A, reorder="rcm")
    assert S.info()["reordered"]
    _attach(D, S, X.CASE_BY_NAME[name])
    _check_info(S, X.CASE_BY_NAME[name])
    assert _same_bits(_factor(S), Lr)
    S.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _jacobi_for(D, A):
    d = np.abs(A.diagonal())
    with np.errstate(all="ignore"):
        dinv = np.where(np.isfinite(1.0 / d), 1.0 / d, 1.0)         # (a diagonal entry may be subnormal in these cases)
    return D.Jacobi(dinv)


def _history(S, b):
    res = S.solve(_dev(b), max_iter=25)
    return np.concatenate((_bits(res.res_history), _bits(res.x.cpu().numpy()))), res.iterations


def _refused(D, S, M, b, status, *texts):
    """Attaching M raises `status` with `texts` in the message; the Jacobi attached before it stays and solves to the same bits."""
    before = _history(S, b)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(M)
    assert e.value.status == status, str(e.value)
    for t in texts:
        assert t in str(e.value), str(e.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    after = _history(S, b)
    assert before[1] == after[1] and np.array_equal(before[0], after[0])
    return str(e.value)


@pytest.mark.parametrize("case", X.ERROR_CASES, ids=lambda c: c.name)
def test_device_refuses_what_the_restatement_refuses(D, case):
    A = case.matrix()
    with pytest.raises(R.FsaiError) as re:
        R.fsai(A, level=case.level)
    assert re.value.kind == case.kind and re.value.column == case.column
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(_jacobi_for(D, A))
    b = O.rhs(A.shape[0], 0)
    if case.kind == "width":
        _refused(D, S, D.FSAI(level=case.level), b, D._lib.ERR_INVALID, f"column {re.value.column} ", f"m = {case.m} ")
    else:
        text = _refused(D, S, D.FSAI(level=case.level), b, D._lib.ERR_PIVOT, f"column {re.value.column}")
        assert text.endswith(f" column {re.value.column}"), text      # (not a longer number that starts with it)
    S.close()


# ---- cache sequences --------------------------------------------------------------------------------------------------------
def _negative_diagonal(A, row):
    B = A.copy()
    k = B.indptr[row] + int(np.searchsorted(B.indices[B.indptr[row]:B.indptr[row + 1]], row))
    assert B.indices[k] == row
    B.data[k] = -B.data[k]
    return B


def test_cache_survives_bad_values_on_the_same_key(D):
    A = E.poisson2d(20)
    bad = _negative_diagonal(A, 137)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(level=2))
    assert not S.fsai_info()["pattern_reused"]
    S.update_values(bad.data)
    with pytest.raises(R.FsaiError) as re:
        R.fsai(bad, level=2)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(level=2))
    assert e.value.status == D._lib.ERR_PIVOT and str(e.value).endswith(f"column {re.value.column}")
    assert S.info()["precond"] == D._lib.PRECOND_NONE                # (update_values dropped the factor; nothing took its place)
    with pytest.raises(D._lib.DpcgError) as e:
        S.fsai_info()
    assert e.value.status == D._lib.ERR_STATE
    S.update_values(A.data)
    S.set_preconditioner(D.FSAI(level=2))
    assert S.fsai_info()["pattern_reused"] and S.fsai_info()["level"] == 2
    assert _same_bits(_factor(S), R.fsai(A, level=2))
    S.close()


def test_cache_survives_a_failure_on_a_fresh_key(D):
    """Two sequences.  Every local system of level 1 is a principal block of one of level 2, so values on which level 2 attaches and
    level 1 fails do not exist: (i) takes the failing level 1 after update_values (which drops the factor, not the cache) and shows
    the level-2 cache by its reuse; (ii) keeps level 2 ATTACHED and fails on a fresh explicit key -- A = poisson2d(20) - 1.5 I is
    indefinite, its level-2 blocks (m <= 7) are positive definite, the 41-wide blocks of a band-40 pattern are not."""
    A = E.poisson2d(20)
    bad = _negative_diagonal(A, 137)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(level=2))
    S.update_values(bad.data)
    with pytest.raises(R.FsaiError) as re:
        R.fsai(bad, level=1)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(level=1))
    assert e.value.status == D._lib.ERR_PIVOT and str(e.value).endswith(f"column {re.value.column}")
    S.update_values(A.data)
    S.set_preconditioner(D.FSAI(level=2))
    assert S.fsai_info()["pattern_reused"] and S.fsai_info()["level"] == 2      # the failed level-1 attach did not replace the cache
    assert _same_bits(_factor(S), R.fsai(A, level=2))
    S.close()

    B = E.csr(E.poisson2d(20) - 1.5 * sp.identity(400))
    P = sp.tril(E.banded_spd(400, 40)).tocsr()
    L2 = R.fsai(B, level=2)
    with pytest.raises(R.FsaiError) as re:
        R.fsai(B, pattern=P)
    assert re.value.kind == "pivot"
    S = D.CsrSystem.from_any(B, reorder=None)
    S.set_preconditioner(D.FSAI(level=2))
    info = S.fsai_info()
    assert _same_bits(_factor(S), L2)
    r = O.rhs(400, 1)
    z = _bits(S.precond_apply(_dev(r)).cpu().numpy())
    for _ in range(2):                                              # (the second failure meets the state the first one left)
        with pytest.raises(D._lib.DpcgError) as e:
            S.set_preconditioner(D.FSAI(pattern=P))
        assert e.value.status == D._lib.ERR_PIVOT and str(e.value).endswith(f"column {re.value.column}")
        assert S.info()["precond"] == D._lib.PRECOND_LLT_MULTIPLY and S.fsai_info() == info
        assert _same_bits(_factor(S), L2)
        assert np.array_equal(_bits(S.precond_apply(_dev(r)).cpu().numpy()), z)
    with pytest.raises(D._lib.DpcgError) as e:                      # ... and a fresh key the symbolic phase refuses (m = 81 > 64)
        S.set_preconditioner(D.FSAI(pattern=sp.tril(E.banded_spd(400, 80)).tocsr()))
    assert e.value.status == D._lib.ERR_INVALID and "column 0 " in str(e.value) and "m = 81" in str(e.value)
    assert S.fsai_info() == info and _same_bits(_factor(S), L2)
    S.set_preconditioner(D.FSAI(level=2))                           # the key that stayed: only values
    assert S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), L2)
    S.close()


def test_same_size_patterns_are_different_keys(D):
    """Two explicit patterns with the same rowptr and nnz that differ in one column: the cache compares the columns too."""
    A = E.poisson2d(20)
    P1 = sp.tril(A).tocsr()
    P1.sort_indices()
    P2 = P1.copy()
    row = 207
    s = P2.indptr[row]
    assert P2.indptr[row + 1] - s == 3 and list(P2.indices[s:s + 3]) == [row - 20, row - 1, row]
    P2.indices[s] = row - 19                                        # (207, 187) moves to (207, 188): still ascending, lower, same sizes
    assert np.array_equal(P1.indptr, P2.indptr) and P1.nnz == P2.nnz and not np.array_equal(P1.indices, P2.indices)
    L1, L2 = R.fsai(A, pattern=P1), R.fsai(A, pattern=P2)
    assert not _same_bits(L1, L2)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(pattern=P1))
    assert not S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), L1)
    S.set_preconditioner(D.FSAI(pattern=P2))
    assert not S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), L2)
    S.set_preconditioner(D.FSAI(pattern=P2))
    assert S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), L2)
    S.set_preconditioner(D.FSAI(pattern=P1))
    assert not S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), L1)
    S.close()


# ---- unsorted A -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson2d_24", "random_bbt_300"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("disorder", ["reversed_rows", "first_two_swapped"])
def test_rows_whose_columns_do_not_ascend(D, name, level, disorder):
    """The solves take unsorted parts; the gather map of FSAI is built by bisection on A's rows.  Either outcome is right: the factor
    of the sorted matrix bit for bit, or DPCG_ERR_INVALID that says "ascending" with the previous preconditioner kept.  (The routine
    refuses.  Before it checked, it searched the unsorted rows: with every row reversed it missed the diagonal and reported a pivot
    error for an SPD matrix; with only two lower entries of a row exchanged it found the diagonal, read the two as absent and
    returned the factor of another matrix with status OK.)"""
    A = E.poisson2d(24) if name == "poisson2d_24" else E.random_bbt(300)
    rp, ci, v = getattr(X, disorder)(A)
    assert not sp.csr_matrix((v, ci, rp), shape=A.shape).has_sorted_indices
    b = O.rhs(A.shape[0], 0)
    S = D.CsrSystem.from_any((rp, ci, v), reorder=None)
    S.set_preconditioner(D.Jacobi(1.0 / A.diagonal()))
    res = S.solve(_dev(b))                                          # the plain solve's tolerance of unsorted parts is unchanged
    r_true = b - A @ res.x.cpu().numpy()
    assert res.status == 0 and np.dot(r_true, r_true) / np.dot(b, b) < 1e-8 * (1 + 1e-6)
    try:
        S.set_preconditioner(D.FSAI(level=level))
    except D._lib.DpcgError as e:
        assert e.status == D._lib.ERR_INVALID and "ascending" in str(e), str(e)
        assert S.info()["precond"] == D._lib.PRECOND_JACOBI
        again = S.solve(_dev(b))
        assert again.iterations == res.iterations and np.array_equal(_bits(again.res_history), _bits(res.res_history))
        assert np.array_equal(_bits(again.x.cpu().numpy()), _bits(res.x.cpu().numpy()))
    else:
        assert _same_bits(_factor(S), R.fsai(A, level=level))
    # an explicit pattern meets the same rows of A
    try:
        S.set_preconditioner(D.FSAI(pattern=sp.tril(A).tocsr()))
    except D._lib.DpcgError as e:
        assert e.status == D._lib.ERR_INVALID and "ascending" in str(e), str(e)
    else:
        assert _same_bits(_factor(S), R.fsai(A, level=1))
    S.close()


# ---- apply and solve through 64-wide rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["banded200_63", "banded200_63_scaled8", "banded200_63_scaled70"])
def test_apply_through_64_wide_rows(D, restated, name):
    """z = L (L^T r): bit for bit what LLtMultiply(restated L) gives, and componentwise within 2 (k + 1) u |L| (|L^T| |r|) of the
    long-double product -- the bound of two dot products of at most k terms each, whatever their summation order (k = the longest
    row of L or L^T).  A plain rtol would mean nothing on the scaled cases: the entries of z span 140 decades."""
    A, Lr = restated(name)
    n = A.shape[0]
    k = int(max(np.diff(Lr.indptr).max(), np.diff(Lr.tocsc().indptr).max()))
    assert k == 64
    r = O.rhs(n, 3)
    S = D.CsrSystem.from_any(A, reorder=None)
    _attach(D, S, X.CASE_BY_NAME[name])
    T = D.CsrSystem.from_any(A, reorder=None)
    T.set_preconditioner(D.LLtMultiply(Lr))
    z = S.precond_apply(_dev(r)).cpu().numpy()
    assert np.array_equal(_bits(z), _bits(T.precond_apply(_dev(r)).cpu().numpy()))
    Ld = Lr.toarray().astype(np.longdouble)
    rl = r.astype(np.longdouble)
    exact = Ld @ (Ld.T @ rl)
    bound = 2 * (k + 1) * U * (np.abs(Ld) @ (np.abs(Ld.T) @ np.abs(rl)))
    assert np.isfinite(z).all() and (bound > 0).all()
    ratio = np.abs(z.astype(np.longdouble) - exact) / bound
    print(f"{name}: worst |z - L L^T r| / bound = {float(ratio.max()):.4f}")
    assert (ratio <= 1).all()
    S.close()
    T.close()


@pytest.mark.parametrize("name", [c.name for c in X.DEGENERATE_CASES])
def test_factor_and_apply_at_degenerate_shapes(D, restated, name):
    """One row, and a diagonal matrix: L = L^T is diagonal, so z_i = l_ii (l_ii r_i) in two roundings whatever the order -- the device's
    L^T (a transpose of one row, of columns whose strictly lower part is empty) must give exactly that."""
    A, Lr = restated(name)
    assert Lr.nnz == A.shape[0]
    r = O.rhs(A.shape[0], 3)
    S = D.CsrSystem.from_any(A, reorder=None)
    _attach(D, S, X.CASE_BY_NAME[name])
    _check_info(S, X.CASE_BY_NAME[name])
    assert _same_bits(_factor(S), Lr)
    z = S.precond_apply(_dev(r)).cpu().numpy()
    assert np.array_equal(_bits(z), _bits(Lr.data * (Lr.data * r)))
    S.close()


def test_solve_through_64_wide_rows(D):
    A = E.banded_spd(1200, 63)
    n = A.shape[0]
    Lr = R.fsai(A, level=1)
    assert np.diff(Lr.indptr).max() == 64
    b = O.rhs(n, 0)
    S = D.CsrSystem.from_any(A, reorder=None)
    T = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    jac = S.solve(_dev(b))
    S.set_preconditioner(D.FSAI(level=1))
    assert S.fsai_info()["columns_by_width"][64] == n - 32 and S.fsai_info()["max_m"] == 64
    T.set_preconditioner(D.LLtMultiply(Lr))
    res, ref = S.solve(_dev(b)), T.solve(_dev(b))
    print(f"banded_spd(1200, 63): jacobi {jac.iterations}, fsai(1) {res.iterations}")
    assert res.status == 0 and ref.status == 0 and res.iterations == ref.iterations
    assert np.array_equal(_bits(res.res_history), _bits(ref.res_history))
    assert np.array_equal(_bits(res.x.cpu().numpy()), _bits(ref.x.cpu().numpy()))
    r_true = b - A @ res.x.cpu().numpy()
    # the recurrence's residual met rtol_sq = 1e-8; the true one differs from it by O(u kappa) of a system with kappa < 200
    assert np.dot(r_true, r_true) / np.dot(b, b) < 1e-8 * (1 + 1e-6)
    assert res.iterations < jac.iterations
    S.close()
    T.close()
