"""CPU checks of the edge-case generators (tests/edge_matrices.py): symmetric, SPD, sorted fp64 CSR, and each reaches the edge it is
named for -- what the device AMG / ILUT edge tests rely on."""

import numpy as np
import pytest
import scipy.sparse as sp

import amg_restatement as R
import edge_matrices as E
import ilut_restatement as IR

SPD = {
    "aniso_1e-3": lambda: E.anisotropic2d(20, 1e-3),
    "aniso_1e-6": lambda: E.anisotropic2d(20, 1e-6),
    "jump2d": lambda: E.jumping((24, 24), 6),
    "jump3d": lambda: E.jumping((8, 8, 8), 2),
    "nine_point": lambda: E.nine_point_mixed(20),
    "bbt": lambda: E.random_bbt(400),
    "identity_rows": lambda: E.boundary_identity(20),
    "three_components": E.three_components,
    "tiny_components": E.tiny_components,
    "stored_zeros": lambda: E.with_stored_zeros(E.poisson2d(20)),
    "hub": lambda: E.hub(20, 150),
    "tiny_1": lambda: E.tiny(1),
    "tiny_17": lambda: E.tiny(17),
    "banded": lambda: E.banded_spd(150, 64),
    "signed_ties": lambda: E.signed_ties(12),
    "candidates": lambda: E.ilut_candidates(194, 60),
}


@pytest.mark.parametrize("name", list(SPD))
def test_generators_give_sorted_symmetric_spd_csr(name):
    A = SPD[name]()
    assert isinstance(A, sp.csr_matrix) and A.dtype == np.float64 and A.has_sorted_indices
    assert A.indices.dtype == np.int32 or A.nnz < 2**31
    assert abs(A - A.T).max() == 0 if A.shape[0] > 1 else True
    assert np.linalg.eigvalsh(A.toarray()).min() > 0


def test_scaled_rows_is_a_congruence_of_the_original():
    A = E.poisson2d(12)
    B = E.scaled_rows(A, seed=3)
    s = np.sqrt(B.diagonal() / A.diagonal())
    assert np.allclose((sp.diags(1 / s) @ B @ sp.diags(1 / s)).toarray(), A.toarray(), rtol=1e-12, atol=0)
    norms = sp.linalg.norm(B, axis=1)
    assert norms.max() / norms.min() > 1e20 and np.array_equal(B.indices, A.indices)


def test_stored_zeros_survive_csr_and_the_restatements():
    A = E.with_stored_zeros(E.poisson2d(16))
    nz = int((A.data == 0).sum())
    assert nz > 50 and int((E.csr(A).data == 0).sum()) == nz
    assert R.strength(A).nnz == R.strength(E.poisson2d(16)).nnz          # a stored zero is never a strong connection
    L, U = IR.ilut(A, 5, 0.0)
    assert (L.data == 0).sum() + (U.data == 0).sum() > 0                  # threshold 0 keeps the zeros the pattern holds


def test_anisotropy_and_jumps_are_what_they_say():
    A = E.anisotropic2d(6, 1e-3)
    assert A[7, 8] == -1e-3 and A[7, 13] == -1.0 and A[7, 7] == 2 + 2e-3
    J = E.jumping((8, 8), 2, 1e6)
    assert J.diagonal().max() / J.diagonal().min() > 1e5
    assert (J - sp.diags(J.diagonal())).max() <= 0                          # an M-matrix of two scales
    N = E.nine_point_mixed(8)
    assert (N - sp.diags(N.diagonal())).max() > 0                           # not an M-matrix
    B = E.random_bbt(200)
    assert (B - sp.diags(B.diagonal())).max() > 0 and (B - sp.diags(B.diagonal())).min() < 0


def test_components_and_identity_rows():
    A = E.tiny_components(10)
    ncomp, lab = sp.csgraph.connected_components(A)
    assert ncomp == 3 and sorted(np.bincount(lab).tolist()) == [1, 2, 100]
    ncomp, lab = sp.csgraph.connected_components(E.three_components())
    assert ncomp == 3 and sorted(np.bincount(lab).tolist()) == [400, 512, 900]
    B = E.boundary_identity(10)
    ident = np.nonzero(B.diagonal() == 1.0)[0]
    assert ident.size > 5 and all(B[i].nnz == 1 and B[:, i].nnz == 1 for i in ident)


def test_hub_row_and_product_counts():
    A = E.hub(12, 40, seed=1)
    n = A.shape[0]
    assert A[n - 1].nnz == 41
    T = sp.csr_matrix((np.ones(n), np.arange(n), np.arange(n + 1)), shape=(n, n))
    assert E.product_counts(A, T)[-1] == 41
    X = sp.random(30, 20, density=0.2, random_state=1, format="csr")
    Y = sp.random(20, 25, density=0.3, random_state=2, format="csr")
    want = [sum(Y[k].nnz for k in X[i].indices) for i in range(30)]
    assert E.product_counts(X, Y).tolist() == want
    Yz = Y.copy()
    Yz.data[:] = 0.0                                                         # structure, not values
    assert np.array_equal(E.pattern_product(X, Yz).indptr, E.pattern_product(X, Y).indptr)


@pytest.mark.parametrize("n_direct,n_fill,positions", [(254, 0, 256), (194, 60, 256), (255, 0, 257), (195, 60, 257)])
def test_ilut_candidate_rows_hold_the_positions_they_say(n_direct, n_fill, positions):
    A = E.ilut_candidates(n_direct, n_fill)
    last = A.shape[0] - 1
    IR.ilut(A, 1, 0.01, cand_cap=positions)
    with pytest.raises(IR.IlutError) as e:
        IR.ilut(A, 1, 0.01, cand_cap=positions - 1)
    assert e.value.kind == "cand" and e.value.row == last
    assert A[last].nnz == n_direct + 2


@pytest.mark.parametrize("hb", [1, 31, 64])
def test_banded_complete_lu_is_the_restatement_at_threshold_0(hb):
    A = E.banded_spd(120, hb, seed=hb)
    L, U = IR.ilut(A, 0, 0.0)
    assert np.abs((L @ U - A).toarray()).max() <= 1e-12 * np.abs(A.toarray()).max()
    assert np.diff(U.indptr).max() == hb + 1


def test_ilut_ties_of_opposite_sign_go_to_the_smaller_column():
    assert IR._select([(7, 1.0), (5, -1.0), (3, 1.0), (9, -2.0)], 2) == [(3, 1.0), (9, -2.0)]
    assert IR._select([(7, 1.0), (5, -1.0), (3, 0.5)], 1) == [(5, -1.0)]
    A = E.signed_ties(6, seed=0)
    off = A.data[A.indices != np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))]
    assert set(np.unique(off).tolist()) == {-1.0, 1.0}                     # equal magnitudes of both signs
