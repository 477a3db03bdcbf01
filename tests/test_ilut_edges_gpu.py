"""ILUT (dpcg_set_precond_ilut) at its capacity edges and beyond M-matrices: the complete LU of banded systems up to the 64-entry
row cap against a dense Doolittle factorisation written here, the 256-position working row (register slots 2 and 3), selection
ties of both signs, stored zeros, rows scaled over 1e+-8, non-M-matrices and tiny systems against tests/ilut_restatement.py bit
for bit, and both applies against scipy."""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import edge_matrices as E
import ilut_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def _attach(D, A, mode="multiply", p=1, threshold=0.1):
    S = D.CsrSystem.from_any(E.csr(A), reorder=None)
    S.set_preconditioner(D.ILUT(mode, add_fill_in=p, threshold=threshold))
    return S


def _same_bits(X, Y):
    return (np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(X.data.view(np.uint64), Y.data.view(np.uint64)))


def doolittle(A: np.ndarray):
    """Dense LU without pivoting, fp64: L unit lower, U upper, A = L U."""
    n = A.shape[0]
    L, U = np.eye(n), np.zeros((n, n))
    for i in range(n):
        U[i, i:] = A[i, i:] - L[i, :i] @ U[:i, i:]
        L[i + 1:, i] = (A[i + 1:, i] - L[i + 1:, :i] @ U[:i, i]) / U[i, i]
    return L, U


@pytest.mark.parametrize("hb", [1, 31, 32, 63, 64])
def test_complete_lu_of_banded_systems(D, hb):
    """threshold 0 and p = 0 keep the whole band (a band LU has no fill outside it): the factor is the complete LU; hb = 64 keeps
    exactly 64 entries in the rows of L and U away from the ends, the cap, and its rows hold 129 positions (slot 2)."""
    A = E.banded_spd(200, hb, seed=hb)
    S = _attach(D, A, p=0, threshold=0.0)
    L, U = S.lu_factors()
    Lr, Ur = R.ilut(A, 0, 0.0)
    assert _same_bits(L, Lr) and _same_bits(U, Ur)
    Ld, Ud = doolittle(A.toarray())
    assert np.linalg.norm(L.toarray() - Ld) <= 1e-12 * np.linalg.norm(Ld)
    assert np.linalg.norm(U.toarray() - Ud) <= 1e-12 * np.linalg.norm(Ud)
    assert np.diff(L.indptr).max() == hb + 1 and np.diff(U.indptr).max() == hb + 1
    r = O.rhs(A.shape[0], 1)
    got = S.precond_apply(torch.from_numpy(r).cuda()).cpu().numpy()
    want = L @ (U @ r)
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    assert np.linalg.norm(got - A @ r) <= 1e-12 * np.linalg.norm(A @ r)        # the complete factor multiplies back to A
    S.close()


def test_band_of_65_exceeds_the_row_cap(D):
    A = E.banded_spd(200, 65, seed=65)
    with pytest.raises(R.IlutError) as e:
        R.ilut(A, 0, 0.0)
    assert e.value.kind == "cap"
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = _attach(D, A, "solve", p=0, threshold=0.1)          # (drops enough to stay under the cap)
    before = S.solve(b, rtol_sq=1e-8, max_iter=100)
    L0, U0 = S.lu_factors()
    with pytest.raises(D._lib.DpcgError) as exc:
        S.set_preconditioner(D.ILUT("multiply", add_fill_in=0, threshold=0.0))
    assert exc.value.status == D._lib.ERR_INVALID and "more than 64 entries" in str(exc.value)
    assert f"row {e.value.row}" in str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_LU_SOLVE
    L1, U1 = S.lu_factors()
    assert _same_bits(L0, L1) and _same_bits(U0, U1)
    after = S.solve(b, rtol_sq=1e-8, max_iter=100)
    assert after.iterations == before.iterations
    assert np.array_equal(after.res_history.view(np.uint64), before.res_history.view(np.uint64))
    S.close()


# (n_direct, n_fill): the last row starts with n_direct + 2 positions and its elimination of column 0 adds n_fill
CAND_256 = [(254, 0), (194, 60)]
CAND_257 = [(255, 0), (195, 60)]


@pytest.mark.parametrize("n_direct,n_fill", CAND_256)
def test_working_row_of_256_positions(D, n_direct, n_fill):
    A = E.ilut_candidates(n_direct, n_fill)
    last = A.shape[0] - 1
    Lr, Ur = R.ilut(A, 1, 0.01)
    with pytest.raises(R.IlutError) as e:
        R.ilut(A, 1, 0.01, cand_cap=255)                    # exactly 256 positions: one fewer allowed fails, at the last row
    assert e.value.kind == "cand" and e.value.row == last
    assert 0 < Lr[last].nnz - 1 < 10                           # most of them fall below tau_i: few are kept
    S = _attach(D, A, p=1, threshold=0.01)
    L, U = S.lu_factors()
    assert _same_bits(L, Lr) and _same_bits(U, Ur)
    S.close()


@pytest.mark.parametrize("n_direct,n_fill", CAND_257)
def test_working_row_of_257_positions_is_refused(D, n_direct, n_fill):
    A = E.ilut_candidates(n_direct, n_fill)
    last = A.shape[0] - 1
    with pytest.raises(R.IlutError) as e:
        R.ilut(A, 1, 0.01)
    assert e.value.kind == "cand" and e.value.row == last
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    before = S.solve(b, rtol_sq=1e-8)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.set_preconditioner(D.ILUT("multiply", add_fill_in=1, threshold=0.01))
    assert exc.value.status == D._lib.ERR_INVALID
    assert "more than 256 positions" in str(exc.value) and f"row {last}" in str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    after = S.solve(b, rtol_sq=1e-8)
    assert after.iterations == before.iterations and torch.equal(after.x, before.x)
    S.close()


SELECTION_MATS = {
    "signed_ties": lambda: E.signed_ties(16),
    "stored_zeros": lambda: E.with_stored_zeros(E.signed_ties(16), seed=1),
    "scaled_rows": lambda: E.scaled_rows(E.poisson2d(16), seed=2),
    "nine_point": lambda: E.nine_point_mixed(16),
    "bbt": lambda: E.random_bbt(300, seed=4),
    "jump2d": lambda: E.jumping((16, 16), 4),
}


@pytest.fixture(scope="module")
def selection_mats():
    return {k: f() for k, f in SELECTION_MATS.items()}


@pytest.mark.parametrize("threshold", [0.0, 1e-4, 0.1])
@pytest.mark.parametrize("p", [0, 1, 2, 5, 16])
@pytest.mark.parametrize("name", list(SELECTION_MATS))
def test_selection_edges_equal_restatement(D, selection_mats, name, p, threshold):
    A = selection_mats[name]
    Lr, Ur = R.ilut(A, p, threshold)
    S = _attach(D, A, p=p, threshold=threshold)
    L, U = S.lu_factors()
    assert _same_bits(L, Lr) and _same_bits(U, Ur)
    S.close()


@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_tiny_systems(D, n):
    A = E.tiny(n)
    for p, threshold in ((0, 0.0), (1, 0.1)):
        Lr, Ur = R.ilut(A, p, threshold)
        S = _attach(D, A, "solve", p=p, threshold=threshold)
        L, U = S.lu_factors()
        assert _same_bits(L, Lr) and _same_bits(U, Ur)
        if threshold == 0.0:                                    # the complete LU: PCG converges at once
            res = S.solve(torch.from_numpy(O.rhs(n, 0)).cuda(), rtol_sq=1e-20)
            assert res.status == 0 and res.iterations <= 2
        S.close()


@pytest.mark.parametrize("name", ["nine_point", "scaled_rows", "stored_zeros", "jump2d"])
def test_applies_equal_scipy(D, selection_mats, name):
    A = selection_mats[name]
    n = A.shape[0]
    Lr, Ur = R.ilut(A, 2, 1e-4)
    r = O.rhs(n, 3)
    rt = torch.from_numpy(r).cuda()
    S = _attach(D, A, "multiply", p=2, threshold=1e-4)
    want = Lr @ (Ur @ r)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    S.set_preconditioner(D.ILUT("solve", add_fill_in=2, threshold=1e-4))
    want = spla.spsolve_triangular(Ur, spla.spsolve_triangular(Lr, r, lower=True), lower=False)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    S.close()
