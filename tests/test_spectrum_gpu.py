"""CsrSystem.spectrum_bounds (dpcg_spectrum: preconditioned Lanczos on the device) against analytic spectra, dense eigenvalues
and a numpy restatement of its recurrence; the harness's kappa beyond kappa_max_n."""

import csv
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle as O
from spectrum_restatement import _hash, _lanczos_numpy  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def _poisson2d_eigs(m):
    c = np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
    return (4 - 2 * c[:, None] - 2 * c[None, :]).ravel()


@pytest.mark.parametrize("kind", ["identity", "jacobi"])
def test_poisson2d_analytic(D, kind):
    S = D.CsrSystem.from_any(O.poisson2d(64))
    S.set_preconditioner(D.Identity() if kind == "identity" else D.Jacobi())
    sb = S.spectrum_bounds()
    lam = _poisson2d_eigs(64) / (1.0 if kind == "identity" else 4.0)
    print(f"poisson2d 64^2 {kind}: {sb.steps} steps, kappa {sb.kappa:.6g}")
    assert sb.converged and sb.steps == len(sb.alpha) == len(sb.beta)
    assert sb.lambda_min == pytest.approx(lam.min(), rel=1e-6)
    assert sb.lambda_max == pytest.approx(lam.max(), rel=1e-6)
    assert sb.kappa == pytest.approx(lam.max() / lam.min(), rel=2e-6)
    assert sb.err_min <= 1e-6 * sb.lambda_min and sb.err_max <= 1e-6 * sb.lambda_max


def test_poisson3d_1m_rows_jacobi(D):
    S = D.CsrSystem.from_any(O.poisson3d(100))
    S.set_preconditioner(D.Jacobi())
    t0 = time.perf_counter()
    sb = S.spectrum_bounds()
    dt = time.perf_counter() - t0
    c = np.cos(np.pi / 101)
    lo, hi = (6 - 6 * c) / 6, (6 + 6 * c) / 6
    print(f"poisson3d 100^3 jacobi: {sb.steps} steps, {dt:.2f} s, kappa {sb.kappa:.6g}")
    assert sb.converged
    assert sb.lambda_min == pytest.approx(lo, rel=1e-6)
    assert sb.lambda_max == pytest.approx(hi, rel=1e-6)


class _DenseSpd:
    """An operator preconditioner (only __matmul__): a dense SPD matrix on the device."""

    def __init__(self, M):
        self.M = M

    def __matmul__(self, r):
        return self.M @ r


def _precond(D, kind, A):
    n = A.shape[0]
    rng = np.random.default_rng(5)
    if kind == "ic0":
        return D.IC0("solve")
    if kind == "ic0-multicolor":
        return D.IC0("solve", ordering="multicolor")
    if kind == "icholt-multiply":
        return D.ICholT("multiply")
    if kind == "llt-random":
        Lr = sp.tril(sp.random(n, n, density=0.01, random_state=3), -1, format="csr") * 0.3
        Lr = (Lr + sp.diags(rng.uniform(0.5, 1.5, n))).tocsr()
        Lr.sort_indices()                              # columns ascending: the diagonal is last in each row
        return D.LLtMultiply(Lr)
    B = rng.standard_normal((n, n)) / np.sqrt(n)
    return D.OperatorPreconditioner(_DenseSpd(torch.from_numpy(B @ B.T + np.eye(n)).cuda()))


@pytest.mark.parametrize("kind", ["ic0", "ic0-multicolor", "icholt-multiply", "llt-random", "operator"])
def test_dense_eigenvalues_small(D, kind):
    A = O.unstructured_like(O.poisson2d(20), 1)
    n = A.shape[0]
    S = D.CsrSystem.from_any(A)
    S.set_preconditioner(_precond(D, kind, A))
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    M = torch.stack([S.precond_apply(eye[:, j]) for j in range(n)], dim=1).cpu().numpy()
    lam = np.sort(np.linalg.eigvals(M @ A.toarray()).real)
    sb = S.spectrum_bounds(max_steps=n, rtol=1e-12)
    assert sb.converged
    assert sb.lambda_min == pytest.approx(lam[0], rel=1e-8)
    assert sb.lambda_max == pytest.approx(lam[-1], rel=1e-8)


def test_first_steps_match_numpy(D):
    A = O.unstructured_like(O.poisson2d(32), 2)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    dinv = O.jacobi_dinv(A)
    sb = S.spectrum_bounds(max_steps=10, rtol=0.0, seed=11)
    a, b = _lanczos_numpy(A, lambda v: dinv * v, 11, 10)
    assert sb.steps == 10 and not sb.converged
    np.testing.assert_allclose(sb.alpha, a, rtol=1e-12)
    np.testing.assert_allclose(sb.beta, b, rtol=1e-12)


def test_numbering_does_not_matter(D):
    A = O.unstructured_like(O.poisson2d(256), 4)         # 65 536 rows in a scattered numbering: "auto" renumbers it
    results = {}
    for mode in ("auto", "none"):
        S = D.CsrSystem.from_any(A, reorder=mode)
        S.set_preconditioner(D.Jacobi())
        results[mode] = (S.reordered, S.spectrum_bounds(max_steps=2000, rtol=1e-7))
        S.close()
    assert results["auto"][0] and not results["none"][0]
    ra, rn = results["auto"][1], results["none"][1]
    assert ra.converged and rn.converged
    assert ra.lambda_min == pytest.approx(rn.lambda_min, rel=1e-9)
    assert ra.lambda_max == pytest.approx(rn.lambda_max, rel=1e-9)


def test_deterministic_and_solve_unaffected(D):
    A = O.poisson2d(48)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A)
    S.set_preconditioner(D.IC0("solve"))
    r1 = S.solve(b)
    s1 = S.spectrum_bounds(seed=3)
    s2 = S.spectrum_bounds(seed=3)
    r2 = S.solve(b)
    assert np.array_equal(s1.alpha, s2.alpha) and np.array_equal(s1.beta, s2.beta)
    assert s1.lambda_min == s2.lambda_min and s1.lambda_max == s2.lambda_max
    assert torch.equal(r1.x, r2.x) and np.array_equal(r1.res_history, r2.res_history)


def test_not_positive_definite_raises(D):
    A = O.poisson2d(16)
    n = A.shape[0]
    S = D.CsrSystem.from_any(A)
    Mneg = sp.diags([np.full(n - 1, 0.1), np.full(n, -1.0), np.full(n - 1, 0.1)], [-1, 0, 1], format="csr")
    S.set_preconditioner(Mneg)                           # a CSR preconditioner with a negative diagonal
    assert isinstance(S._precond, D.CsrPreconditioner)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds()
    assert exc.value.status == D._lib.BREAKDOWN


def test_oversize_basis_raises_nomem(D):
    S = D.CsrSystem.from_any(O.poisson3d(100))
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds(max_steps=1_000_000)          # 2 x 1 000 001 x 1e6 doubles: 16 TB
    assert exc.value.status == D._lib.ERR_NOMEM and "basis" in str(exc.value)


def test_harness_kappa_beyond_kappa_max_n(D, tmp_path):
    from deeppreconditioning_amd.benchmark_suite import BenchmarkSuite, ListDataSet
    A = O.poisson2d(20)
    data = ListDataSet([A], [O.rhs(A.shape[0], 0)])
    runs = {}
    for cap in (100, 3000):
        suite = BenchmarkSuite(data, None, techniques=("vanilla", "jacobi"), results_directory=tmp_path / str(cap), kappa_max_n=cap)
        suite.run()
        suite.dump_csv()
        runs[cap] = suite
    lz, dense = runs[100], runs[3000]
    for t in ("vanilla", "jacobi"):
        assert lz.kappa_sources[t] == ["lanczos"] and dense.kappa_sources[t] == ["dense"]
        assert lz.kappas[t][0] == pytest.approx(dense.kappas[t][0], rel=1e-6)
        assert np.isnan(lz.densities[t][0])
    with (tmp_path / "100" / "kappa_sources.csv").open() as f:
        assert list(csv.reader(f)) == [["vanilla", "jacobi"], ["lanczos", "lanczos"]]
    assert not (tmp_path / "3000" / "kappa_sources.csv").exists()
