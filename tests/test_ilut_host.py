"""CPU checks of the ILUT contract (tests/ilut_restatement.py) and of ILUT's argument validation."""

import numpy as np
import pytest
import scipy.sparse as sp

import ilut_restatement as R


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n)


def test_no_dropping_is_the_complete_lu():
    A = _spd(9, 0)
    L, U = R.ilut(sp.csr_matrix(A), add_fill_in=9, threshold=0.0)
    # Doolittle LU without pivoting (an SPD matrix needs none)
    n = A.shape[0]
    Lr, Ur = np.eye(n), np.zeros((n, n))
    for i in range(n):
        Ur[i, i:] = A[i, i:] - Lr[i, :i] @ Ur[:i, i:]
        Lr[i + 1:, i] = (A[i + 1:, i] - Lr[i + 1:, :i] @ Ur[:i, i]) / Ur[i, i]
    assert np.max(np.abs(L.toarray() - Lr)) < 1e-13
    assert np.max(np.abs(U.toarray() - Ur)) < 1e-13 * np.max(np.abs(Ur))
    assert np.max(np.abs((L @ U).toarray() - A)) < 1e-13 * np.max(np.abs(A))


def test_tridiagonal_is_exact_without_fill():
    n = 12
    A = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    L, U = R.ilut(A, add_fill_in=0, threshold=0.0)
    assert L.nnz == 2 * n - 1 and U.nnz == 2 * n - 1
    assert np.max(np.abs((L @ U - A).toarray())) < 1e-14


def test_layout_diagonal_last_in_l_first_in_u():
    from oracle import oracle as O
    L, U = R.ilut(O.poisson2d(8), add_fill_in=1, threshold=0.1)
    for i in range(64):
        lr = L.indices[L.indptr[i]:L.indptr[i + 1]]
        ur = U.indices[U.indptr[i]:U.indptr[i + 1]]
        assert lr[-1] == i and L.data[L.indptr[i + 1] - 1] == 1.0 and np.all(np.diff(lr) > 0) and np.all(lr <= i)
        assert ur[0] == i and np.all(np.diff(ur) > 0) and np.all(ur >= i)


def test_hand_derived_5x5():
    A = np.array([[4.0, 2.0, 2.0, 1.5, 0.0],
                  [2.0, 4.0, 0.0, 1.75, 0.0],
                  [2.0, 0.0, 4.0, 0.0, 1.0],
                  [1.5, 1.75, 0.0, 4.0, 1.0],
                  [0.0, 0.0, 1.0, 1.0, 4.0]])
    L, U = R.ilut(sp.csr_matrix(A), add_fill_in=0, threshold=0.1)
    # row 1 (tau = 0.1 sqrt(23.0625)): w_0 = 2 / 4 = 0.5; w_1 = 4 - 0.5 * 2 = 3, fill w_2 = -1, w_3 = 1.75 - 0.5 * 1.5 = 1.
    #   p_U = 1 and |w_2| = |w_3|: the TIE goes to the smaller column -- the fill at 2 stays, A's own entry at 3 goes
    # row 2 (tau = 0.1 sqrt(21)): w_0 = 0.5; fill w_1 = -1, w_2 = 3, fill w_3 = -0.75; w_1 / U_11 = -1/3 is below TAU: dropped;
    #   U part: |w_4| = 1 > |w_3| = 0.75 >= tau, p_U = 1: the fill at 3 is dropped by the COUNT
    # row 3 (tau = 0.1 sqrt(23.3125)): w_0 = 1.5 / 4 = 0.375 < tau: dropped; w_1 = 1.75 / 3 kept; fill w_2 = 1.75 / 3 then
    #   divided by U_22 = 3: below tau, dropped; w_3 = 4 (U row 1 kept nothing at 3); row 4: both L entries below tau
    Le = np.eye(5)
    Le[1, 0] = Le[2, 0] = 0.5
    Le[3, 1] = 1.75 / 3.0
    Ue = np.array([[4.0, 2.0, 2.0, 1.5, 0.0],
                   [0.0, 3.0, -1.0, 0.0, 0.0],
                   [0.0, 0.0, 3.0, 0.0, 1.0],
                   [0.0, 0.0, 0.0, 4.0, 1.0],
                   [0.0, 0.0, 0.0, 0.0, 4.0]])
    assert np.array_equal(L.toarray(), Le)
    assert np.array_equal(U.toarray(), Ue)
    # with room for two more entries per row both count-dropped entries come back (the tie and the count were what decided)
    L2, U2 = R.ilut(sp.csr_matrix(A), add_fill_in=2, threshold=0.1)
    assert U2[1, 3] == 1.0 and U2[2, 3] == -0.75
    assert L2[2, 1] == 0.0                # (the tau drop does not depend on the count)


def test_zero_pivot_and_caps_raise():
    A = sp.csr_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]))
    with pytest.raises(R.IlutError) as e:
        R.ilut(A, add_fill_in=1, threshold=0.0)
    assert e.value.kind == "pivot" and e.value.row == 1
    n = 80                                                   # an arrow: row 0 keeps 79 entries of U
    A = sp.lil_matrix((n, n))
    A.setdiag(100.0)
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    with pytest.raises(R.IlutError) as e:
        R.ilut(A.tocsr(), add_fill_in=0, threshold=0.0)
    assert e.value.kind == "cap" and e.value.row == 0
    n = 300                                                  # a row of 300 positions
    A = sp.lil_matrix((n, n))
    A.setdiag(1000.0)
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    with pytest.raises(R.IlutError) as e:
        R.ilut(A.tocsr(), add_fill_in=0, threshold=0.0)
    assert e.value.kind == "cand" and e.value.row == 0


def test_ilut_validates_before_any_library_call(monkeypatch):
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import _lib

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    for kw in ({"mode": "bogus"}, {"add_fill_in": -1}, {"threshold": -0.5}, {"threshold": float("nan")}):
        with pytest.raises(ValueError):
            D.ILUT(**kw)
    M = D.ILUT("solve", add_fill_in=2, threshold=0.0)
    assert M.mode == _lib.PRECOND_LU_SOLVE and (M.add_fill_in, M.threshold) == (2, 0.0)
    assert D.ILUT().mode == _lib.PRECOND_LU_MULTIPLY


def test_harness_maps_incomplete_lu():
    from deeppreconditioning_amd import benchmark_suite as B
    suite = B.BenchmarkSuite.__new__(B.BenchmarkSuite)
    M = suite._construct("incomplete_lu", None, None, 0)
    assert type(M).__name__ == "ILUT" and (M.add_fill_in, M.threshold) == (1, 0.1)
    assert "ilupp" in B.COMPARABILITY["incomplete_lu"] and "incomplete_lu" not in B.BenchmarkSuite.techniques
