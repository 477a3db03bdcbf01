"""ILUT (dpcg_set_precond_ilut): the device factors against the numpy restatement (tests/ilut_restatement.py) bit for bit, both
applies, solves, graph replay, reuse after update_values, errors, isolation from ICholT and the harness's `incomplete_lu` row."""

import csv

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import ilut_restatement as R
from deeppreconditioning_amd import meshes
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PARAMS = [(1, 0.1), (2, 0.01)]          # the harness's arguments, and a setting that keeps fill in L as well


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def systems():
    """Built once per module: the reference's two sizes (2.3K and ~23K rows) and one between."""
    return {
        "poisson2d_48": O.poisson2d(48),
        "poisson2d_64": O.poisson2d(64),
        "quadtree": meshes.quadtree_fv_laplacian(150, 5),
        "quadtree_random": meshes.quadtree_fv_laplacian(150, 5, numbering="random"),
    }


@pytest.fixture(scope="module")
def restated(systems):
    cache = {}

    def get(name, params):
        if (name, params) not in cache:
            cache[(name, params)] = R.ilut(_csr(systems[name]), *params)
        return cache[(name, params)]
    return get


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def _attach(D, A, mode="multiply", params=(1, 0.1), reorder=None):
    S = D.CsrSystem.from_any(_csr(A), reorder=reorder)
    S.set_preconditioner(D.ILUT(mode, add_fill_in=params[0], threshold=params[1]))
    return S


def _same_bits(X, Y):
    return (np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(X.data.view(np.uint64), Y.data.view(np.uint64)))


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name", ["poisson2d_48", "poisson2d_64", "quadtree", "reordered"])
def test_factors_equal_restatement(D, systems, restated, name, params):
    src = "quadtree_random" if name == "reordered" else name
    S = _attach(D, systems[src], params=params, reorder="rcm" if name == "reordered" else None)
    assert S.reordered == (name == "reordered")
    L, U = S.lu_factors()
    Lr, Ur = restated(src, params)
    assert _same_bits(L, Lr) and _same_bits(U, Ur)
    info = S.info()
    assert info["precond"] == D._lib.PRECOND_LU_MULTIPLY and info["precond_nnz"] == L.nnz + U.nnz
    if params == (2, 0.01):
        assert L.nnz > 2 * L.shape[0]           # (the L part is exercised, fill included)
    S.close()


@pytest.mark.parametrize("reorder", [None, "rcm"])
def test_applies(D, systems, restated, reorder):
    A = systems["quadtree_random"]
    Lr, Ur = restated("quadtree_random", (2, 0.01))
    r = O.rhs(A.shape[0], 3)
    rt = torch.from_numpy(r).cuda()
    S = _attach(D, A, "multiply", (2, 0.01), reorder)
    want = Lr @ (Ur @ r)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-14 * np.linalg.norm(want)
    S.set_preconditioner(D.ILUT("solve", add_fill_in=2, threshold=0.01))
    assert S.info()["precond"] == D._lib.PRECOND_LU_SOLVE and S.info()["levels_upper"] > 1
    y = spla.spsolve_triangular(Lr, r, lower=True)
    want = spla.spsolve_triangular(Ur, y, lower=False)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    got_u = S.sptrsv(rt, upper=True).cpu().numpy()
    want_u = spla.spsolve_triangular(Ur, r, lower=False)
    assert np.linalg.norm(got_u - want_u) <= 1e-12 * np.linalg.norm(want_u)
    S.close()


@pytest.mark.parametrize("mode", ["multiply", "solve"])
def test_solve_history_and_graph_replay(D, systems, mode):
    A = _csr(systems["poisson2d_48"])
    b = O.rhs(A.shape[0], 0)
    bt = torch.from_numpy(b).cuda()
    S = _attach(D, A, mode, (2, 0.01))
    L, U = S.lu_factors()
    # M = L U multiplied is the reference's use: M ~ A, so PCG squares the condition number and a short run is compared
    max_iter = 100 if mode == "multiply" else 1024
    res = S.solve(bt, rtol_sq=1e-8, max_iter=max_iter)
    if mode == "multiply":
        _, it, hist, _ = O.preconditioned_conjugate_gradient(A, b, (L @ U).tocsr(), rtol=1e-8, max_iter=max_iter)
        assert res.iterations == it
        np.testing.assert_allclose(res.res_history, hist, rtol=1e-10, atol=0)
    else:
        _, it, hist, _ = O.preconditioned_conjugate_gradient(A, b, _LuSolve(L, U), rtol=1e-8, max_iter=max_iter)
        assert res.status == 0 and abs(res.iterations - it) <= 1, (res.iterations, it)
    ng = S.solve(bt, rtol_sq=1e-8, max_iter=max_iter, flags=D._lib.NO_GRAPH)
    again = S.solve(bt, rtol_sq=1e-8, max_iter=max_iter)
    for other in (ng, again):
        assert other.iterations == res.iterations
        assert np.array_equal(other.res_history.view(np.uint64), res.res_history.view(np.uint64))
        assert np.array_equal(other.x.cpu().numpy().view(np.uint64), res.x.cpu().numpy().view(np.uint64))
    S.close()


class _LuSolve:
    def __init__(self, L, U):
        self.L, self.U = L, U

    def __matmul__(self, r):
        return spla.spsolve_triangular(self.U, spla.spsolve_triangular(self.L, r, lower=True), lower=False)


def test_update_values_then_ilut_equals_fresh(D, systems):
    A = _csr(systems["quadtree"])
    S = _attach(D, A, params=(2, 0.01))
    S.update_values(torch.from_numpy(2.0 * A.data).cuda())
    with pytest.raises(D._lib.DpcgError):
        S.lu_factors()                                   # the factor was dropped with the old values
    S.set_preconditioner(D.ILUT("multiply", add_fill_in=2, threshold=0.01))
    F = _attach(D, 2.0 * A, params=(2, 0.01))
    for X, Y in zip(S.lu_factors(), F.lu_factors()):
        assert _same_bits(X, Y)
    b = torch.from_numpy(O.rhs(A.shape[0], 1)).cuda()
    r1, r2 = S.solve(b, rtol_sq=1e-8, max_iter=100), F.solve(b, rtol_sq=1e-8, max_iter=100)
    assert np.array_equal(r1.res_history.view(np.uint64), r2.res_history.view(np.uint64))
    S.close()
    F.close()


def test_errors_keep_the_previous_preconditioner(D):
    bad = sp.csr_matrix(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]))     # row 1: w_1 = 1 - 1 = 0
    A = _csr(sp.block_diag((O.poisson2d(8), bad)))
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    before = S.solve(b, rtol_sq=1e-8, max_iter=50)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.set_preconditioner(D.ILUT("multiply", add_fill_in=1, threshold=0.0))
    assert exc.value.status == D._lib.ERR_PIVOT and "row 65" in str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    after = S.solve(b, rtol_sq=1e-8, max_iter=50)
    assert after.iterations == before.iterations
    assert np.array_equal(after.res_history.view(np.uint64), before.res_history.view(np.uint64))
    S.close()
    n = 80                                               # an arrow: row 0 would keep 79 entries of U
    W = sp.lil_matrix((n, n))
    W.setdiag(100.0)
    W[0, 1:] = 1.0
    W[1:, 0] = 1.0
    S = D.CsrSystem.from_any(_csr(W), reorder=None)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.set_preconditioner(D.ILUT("solve", add_fill_in=0, threshold=0.0))
    assert exc.value.status == D._lib.ERR_INVALID
    S.close()


def test_spectrum_refused_and_icholt_after_ilut(D, systems):
    A = _csr(systems["poisson2d_48"])
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = _attach(D, A, "solve", (2, 0.01))
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds()
    assert exc.value.status == D._lib.BREAKDOWN and "not symmetric" in str(exc.value)
    S.solve(b, rtol_sq=1e-8)
    S.set_preconditioner(D.ICholT("multiply"))
    F = D.CsrSystem.from_any(A, reorder=None)
    F.set_preconditioner(D.ICholT("multiply"))
    r1, r2 = S.solve(b, rtol_sq=1e-8), F.solve(b, rtol_sq=1e-8)
    assert r1.iterations == r2.iterations and np.array_equal(r1.res_history, r2.res_history)
    assert np.array_equal(r1.x.cpu().numpy(), r2.x.cpu().numpy())
    S.close()
    F.close()


def test_harness_row(D, tmp_path):
    from deeppreconditioning_amd.benchmark_suite import BenchmarkSuite, ListDataSet
    mats = [O.poisson2d(16), O.poisson2d(20)]
    data = ListDataSet(mats, [O.rhs(m.shape[0], 0) for m in mats])
    suite = BenchmarkSuite(data, None, techniques=("jacobi", "incomplete_lu"), results_directory=tmp_path)
    suite.run()
    suite.dump_csv()
    with (tmp_path / "table.csv").open() as f:
        rows = {r[0]: r for r in csv.reader(f)}
    assert "incomplete_lu" in rows and np.isfinite(float(rows["incomplete_lu"][3]))
    with (tmp_path / "comparability.csv").open() as f:
        comp = {r[0]: r[1] for r in csv.reader(f)}
    assert "ILUT" in comp["incomplete_lu"] and "unpinned" in comp["incomplete_lu"]
    assert all(np.isfinite(v) for v in suite.iterations["incomplete_lu"])


def test_262k_rows_factor_and_strip_scheduled_solves(D):
    # beyond 131 072 rows the solve schedules try the strip plan first (schedule_factor): U's strips come from U's own pattern
    A = _csr(O.poisson2d(512))
    Lr, Ur = R.ilut(A, 1, 0.1)
    r = O.rhs(A.shape[0], 3)
    rt = torch.from_numpy(r).cuda()
    S = _attach(D, A, "solve", (1, 0.1))
    L, U = S.lu_factors()
    assert _same_bits(L, Lr) and _same_bits(U, Ur)
    want = spla.spsolve_triangular(Ur, spla.spsolve_triangular(Lr, r, lower=True), lower=False)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
    S.set_preconditioner(D.ILUT("multiply", add_fill_in=1, threshold=0.1))
    want = Lr @ (Ur @ r)
    got = S.precond_apply(rt).cpu().numpy()
    assert np.linalg.norm(got - want) <= 1e-14 * np.linalg.norm(want)
    S.close()
