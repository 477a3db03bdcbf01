"""PCG with a null-space projection as restated in tests/nullspace_restatement.py (CPU): it converges on the singular
pure-Neumann systems the device tests use, returns the minimum-norm solution (Z^T x = 0), and the unprojected loop -- what a
handle without a null space runs -- does not converge on them.  b = default_rng(1).random(n) is deliberately inconsistent.

Bounds.  Z^T x: the final projection leaves k sums of n products rounded to eps = 2^-53: |Z^T x| <= n eps ||x||.  The true
residual ||P b - A x||^2 / ||P b||^2 of a converged run: the recurrence's <r,r>/<b',b'> is below rtol_sq = 1e-8 and drifts from
the true one by rounding only; 2 rtol_sq leaves a factor two for that.
"""

import pathlib
import re

import numpy as np
import pytest
import scipy.sparse as sp

import nullspace_restatement as R
from deeppreconditioning_amd.poisson import neumann_csr

EPS = 2.0 ** -53
ROOT = pathlib.Path(__file__).resolve().parent.parent


def two_block():
    A = sp.block_diag([neumann_csr((8, 8), 2), neumann_csr((6, 10), 2)], format="csr")
    Z = np.zeros((124, 2))
    Z[:, 0] = 1.0
    Z[:64, 1] = 1.0
    return sp.csr_matrix(A), Z


SYSTEMS = {
    "16x16": lambda: (neumann_csr((16, 16)), np.ones((256, 1))),
    "12x10_s3": lambda: (neumann_csr((12, 10), 3), np.ones((120, 1))),
    "8x8x8": lambda: (neumann_csr((8, 8, 8)), np.ones((512, 1))),
    "9x7x5_s5": lambda: (neumann_csr((9, 7, 5), 5), np.ones((315, 1))),
    "two_block": two_block,
    "130x127": lambda: (neumann_csr((130, 127)), np.ones((130 * 127, 1))),
}


def test_neumann_csr_is_a_symmetric_graph_laplacian():
    for dims, seed in (((5, 4), None), ((4, 3, 2), 7)):
        A = neumann_csr(dims, seed)
        n = int(np.prod(dims))
        assert A.shape == (n, n) and A.indices.dtype == np.int32 and A.has_sorted_indices
        assert abs(A - A.T).max() == 0.0
        assert np.abs(A @ np.ones(n)).max() <= 8 * EPS * abs(A).sum(axis=1).max()
        off = A - sp.diags(A.diagonal())
        assert off.nnz == 2 * sum(n // d * (d - 1) for d in dims) and off.data.max() < 0.0
        if seed is None:
            assert set(np.unique(off.data)) == {-1.0}
        else:
            assert 0.1 <= -off.data.max() and -off.data.min() <= 10.0
    ev = np.linalg.eigvalsh(neumann_csr((5, 4)).toarray())
    assert abs(ev[0]) < 1e-12 and ev[1] > 0.05            # one zero eigenvalue: semi-definite, the kernel is the constants


@pytest.mark.parametrize("pre", ["identity", "jacobi"])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_projected_loop_converges_and_plain_loop_does_not(name, pre):
    A, Zraw = SYSTEMS[name]()
    n = A.shape[0]
    Z = R.orthonormalise(Zraw)
    assert np.abs(Z.T @ Z - np.eye(Z.shape[1])).max() <= 1e-14
    b = np.random.default_rng(1).random(n)
    m = R.jacobi(A) if pre == "jacobi" else None
    status, k, hist, x = R.pcg(A, b, Z, m)
    assert status == R.OK and len(hist) == k + 1 and hist[-1] < 1e-8 and k < 1024
    assert np.abs(Z.T @ x).max() <= n * EPS * np.linalg.norm(x)
    assert R.true_residual(A, b, Z, x) <= 2e-8
    status, k, hist, _ = R.pcg(A, b, None, m)
    assert status == R.MAX_ITER and k == 1024 and hist.min() > 1e-2


def test_constant_alone_does_not_serve_two_regions():
    A, Zraw = two_block()
    b = np.random.default_rng(1).random(124)
    status, k, hist, _ = R.pcg(A, b, R.constant(124), None)
    assert status == R.MAX_ITER and k == 1024 and hist.min() > 1e-4
    assert R.pcg(A, b, R.orthonormalise(Zraw), None)[0] == R.OK


def test_start_from_x0_and_cap():
    A, Zraw = SYSTEMS["16x16"]()
    Z = R.orthonormalise(Zraw)
    rng = np.random.default_rng(1)
    b = rng.random(256)
    _, _, _, x_none = R.pcg(A, b, Z, R.jacobi(A))
    status, _, _, x_x0 = R.pcg(A, b, Z, R.jacobi(A), x0=rng.random(256))
    assert status == R.OK
    ev = np.linalg.eigvalsh(A.toarray())
    kappa_eff = ev[-1] / ev[1]
    assert np.linalg.norm(x_x0 - x_none) <= 10 * 1e-4 * kappa_eff * np.linalg.norm(x_none)
    status, k, _, x = R.pcg(A, b, Z, R.jacobi(A), max_iter=5)
    assert status == R.MAX_ITER and k == 5 and np.abs(Z.T @ x).max() <= 256 * EPS * np.linalg.norm(x)


def test_orthonormalise_refuses_dependent_columns():
    with pytest.raises(ValueError):
        R.orthonormalise(np.ones((10, 2)))


def test_header_declares_and_bindings_bind():
    from deeppreconditioning_amd import _lib
    header = (ROOT / "include" / "dpcg.h").read_text()
    assert re.search(r"int dpcg_set_nullspace\(dpcg_handle_t h, int k, const double \*Z, int memspace, double check_tol, dpcg_stream_t stream\);", header)
    assert re.search(r"int dpcg_get_nullspace\(dpcg_handle_t h, int \*k, double \*Z_host\);", header)
    assert len(_lib.SIGNATURES["dpcg_set_nullspace"][1]) == 6 and len(_lib.SIGNATURES["dpcg_get_nullspace"][1]) == 3
    makefile = (ROOT / "deeppreconditioning_amd" / "csrc" / "Makefile").read_text()
    assert "dpcg_nullspace.hip" in makefile
