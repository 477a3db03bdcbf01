"""CPU checks of the AMG smoothers' contract (tests/amg_smoother_restatement.py) and of SmoothedAggregation's new arguments."""

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

import amg_restatement as R
import amg_smoother_restatement as SR
from deeppreconditioning_amd import meshes
from oracle import oracle as O

SMOOTHERS = (SR.JACOBI, SR.GAUSS_SEIDEL, SR.CHEBYSHEV)


def _permuted(A, colors):
    perm = np.concatenate(SR.color_classes(colors))
    Q = sp.csr_matrix(A)[perm][:, perm].tocsr()
    return perm, Q


@pytest.mark.parametrize("A", [O.poisson2d(12), O.unstructured_like(O.poisson2d(10), seed=4)])
def test_forward_sweep_is_gauss_seidel_in_colour_order(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    colors = SR.greedy_colors(A)
    assert SR.is_proper(A, colors)
    classes = SR.color_classes(colors)
    perm, Q = _permuted(A, colors)
    rng = np.random.default_rng(0)
    b, x0 = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    dinv = 1.0 / A.diagonal()
    x = x0.copy()
    for rows in classes:                               # forward: the passes 0 .. m-1
        SR.gs_pass(A, dinv, b, x, rows)
    DL = sp.tril(Q, format="csr")
    xf = x0[perm] + spsolve_triangular(DL, b[perm] - Q @ x0[perm], lower=True)
    assert np.allclose(x[perm], xf, rtol=1e-13, atol=1e-13)
    # the symmetric sweep = forward, then its transpose (the backward sweep, (D + U)^-1); pass m-1 is not repeated
    xs = SR.gs_sweep(A, dinv, b, x0.copy(), classes)
    DU = sp.triu(Q, format="csr")
    xb = xf + spsolve_triangular(DU, b[perm] - Q @ xf, lower=False)
    assert np.allclose(xs[perm], xb, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("kind", SMOOTHERS)
@pytest.mark.parametrize("name", ["poisson2d_32", "quadtree"])
def test_cycle_is_symmetric_positive_definite(kind, name):
    A = O.poisson2d(32) if name == "poisson2d_32" else meshes.quadtree_fv_laplacian(30, 3)
    H = R.hierarchy(A, max_coarse=50)
    assert len(H.levels) >= 3
    for sweeps in (1, 2):
        M = SR.dense_operator(H, SR.smoothers_for(H, kind), sweeps)
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
        assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0


def test_jacobi_restatement_is_the_original_cycle():
    A = O.poisson2d(20)
    H = R.hierarchy(A, max_coarse=30)
    b = O.rhs(A.shape[0], 0)
    for sweeps in (1, 2):
        H.sweeps = sweeps
        ref = R.vcycle(H, b)
        got = SR.vcycle(H, SR.smoothers_for(H, SR.JACOBI), b, sweeps)
        assert np.linalg.norm(got - ref) <= 1e-13 * np.linalg.norm(ref)


@pytest.mark.parametrize("degree", range(1, 9))
def test_chebyshev_residual_polynomial(degree):
    u, ratio = 1.7, 30.0
    c1, c2, lo, hi = SR.chebyshev_coefficients(u, degree, ratio)
    assert (lo, hi) == (u / ratio, u)
    lam = np.linspace(0.0, u, 4001)
    A = sp.diags(lam).tocsr()                            # D = I: the smoother is x = p(lambda) b
    x = SR.chebyshev(A, np.ones_like(lam), np.ones_like(lam), np.zeros_like(lam), c1, c2)
    res = 1.0 - lam * x                                  # the residual polynomial 1 - lambda p(lambda)
    assert np.all(np.abs(res) <= 1.0 + 1e-12)
    theta, delta = (u + lo) / 2, (u - lo) / 2
    T = np.polynomial.chebyshev.Chebyshev.basis(degree)
    inside = lam >= lo
    cheb = T((theta - lam[inside]) / delta) / T(theta / delta)
    assert np.abs(res[inside] - cheb).max() <= 1e-12
    assert np.abs(res[inside]).max() <= 1.0 / T(theta / delta) + 1e-12


@pytest.mark.parametrize("A", [O.poisson2d(64), O.poisson3d(16)])
def test_gauss_seidel_needs_no_more_iterations_than_jacobi(A):
    b = O.rhs(A.shape[0], 0)
    H = R.hierarchy(A)
    its = {}
    for kind in (SR.JACOBI, SR.GAUSS_SEIDEL):
        _, its[kind], _, _ = O.preconditioned_conjugate_gradient(A, b, SR.VCycle(H, SR.smoothers_for(H, kind), 1), rtol=1e-8)
    assert its[SR.GAUSS_SEIDEL] <= its[SR.JACOBI], its


@pytest.mark.parametrize("kw", [dict(smoother="sor"), dict(smoother=None), dict(smoother="chebyshev", degree=0),
                                dict(smoother="chebyshev", degree=9), dict(degree=2.5), dict(eig_ratio=1.0), dict(eig_ratio=0.5),
                                dict(eig_ratio=float("inf")), dict(eig_ratio=float("nan"))])
def test_smoothed_aggregation_rejects_bad_smoother_arguments(kw):
    from deeppreconditioning_amd import SmoothedAggregation
    with pytest.raises(ValueError):
        SmoothedAggregation(**kw)


def test_smoothed_aggregation_smoother_arguments():
    from deeppreconditioning_amd import SmoothedAggregation
    d = SmoothedAggregation()
    assert (d.smoother, d.degree, d.eig_ratio) == ("jacobi", 2, 30.0)
    c = SmoothedAggregation(smoother="chebyshev", degree=3, eig_ratio=10)
    assert (c.smoother, c.degree, c.eig_ratio) == ("chebyshev", 3, 10.0)
    assert SmoothedAggregation(smoother="gauss_seidel", sweeps=2).smoother == "gauss_seidel"


def test_harness_knows_both_smoothers_and_keeps_its_defaults():
    from deeppreconditioning_amd.benchmark_suite import COMPARABILITY, BenchmarkSuite
    default = BenchmarkSuite.__dataclass_fields__["techniques"].default
    assert default == ("vanilla", "jacobi", "incomplete_cholesky", "incomplete_cholesky_solve", "learned")
    for name in ("algebraic_multigrid_gauss_seidel", "algebraic_multigrid_chebyshev"):
        assert name in COMPARABILITY and name not in default
    assert "Gauss-Seidel" in COMPARABILITY["algebraic_multigrid_gauss_seidel"]
    assert "Chebyshev" in COMPARABILITY["algebraic_multigrid_chebyshev"]
