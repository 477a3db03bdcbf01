"""FSAI (dpcg_set_precond_fsai / dpcg_set_precond_fsai_pattern): the device factor against the numpy restatement
(tests/fsai_restatement.py) bit for bit in every width class, the explicit pattern, the apply and the solves against
LLtMultiply(restated L) bit for bit, reuse after update_values, the errors, the spectrum and the harness rows."""

import csv

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fsai_restatement as R
from deeppreconditioning_amd import meshes
from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (system, level): every width class of the device kernels is hit (asserted in test_every_width_class_is_hit)
FACTOR_CASES = ([(s, l) for s in ("poisson2d_48", "poisson2d_256", "poisson3d_40", "quadtree", "quadtree_random") for l in (1, 2, 3)]
                + [("delaunay_20000", 1), ("delaunay_4000", 2)])
EXPECTED_MAX_M = {("poisson2d_48", 1): 3, ("poisson2d_48", 2): 7, ("poisson2d_48", 3): 13, ("poisson2d_256", 1): 3,
                  ("poisson2d_256", 2): 7, ("poisson2d_256", 3): 13, ("poisson3d_40", 1): 4, ("poisson3d_40", 2): 13,
                  ("poisson3d_40", 3): 32, ("quadtree", 1): 9, ("quadtree", 2): 19, ("quadtree", 3): 33, ("quadtree_random", 1): 8,
                  ("quadtree_random", 2): 20, ("quadtree_random", 3): 38, ("delaunay_20000", 1): 14, ("delaunay_4000", 2): 51}


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


@pytest.fixture(scope="module")
def systems():
    return {
        "poisson2d_48": _csr(O.poisson2d(48)),
        "poisson2d_256": _csr(O.poisson2d(256)),
        "poisson3d_40": _csr(O.poisson3d(40)),
        "quadtree": _csr(meshes.quadtree_fv_laplacian(150, 5)),
        "quadtree_random": _csr(meshes.quadtree_fv_laplacian(150, 5, numbering="random")),
        "delaunay_20000": _csr(meshes.delaunay_laplacian(20000, 0)),
        "delaunay_4000": _csr(meshes.delaunay_laplacian(4000, 0)),
    }


@pytest.fixture(scope="module")
def restated(systems):
    cache = {}

    def get(name, level):
        if (name, level) not in cache:
            cache[(name, level)] = R.fsai(systems[name], level=level)
        return cache[(name, level)]
    return get


def _dev(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda()


def _factor(S):
    rp, ci, v = S.factor()
    return sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))


def _same_bits(X, Y):
    return (np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(X.data.view(np.uint64), Y.data.view(np.uint64)))


@pytest.mark.parametrize("name,level", FACTOR_CASES)
def test_factor_equals_restatement(D, systems, restated, name, level):
    S = D.CsrSystem.from_any(systems[name], reorder=None)
    S.set_preconditioner(D.FSAI(level=level))
    info = S.fsai_info()
    counts, max_m = R.width_class_counts(systems[name], level=level)
    assert info["level"] == level and info["max_m"] == max_m == EXPECTED_MAX_M[(name, level)]
    assert [info["columns_by_width"][w] for w in R.WIDTH_CLASSES] == counts
    assert not info["pattern_reused"]
    assert S.info()["precond"] == D._lib.PRECOND_LLT_MULTIPLY and S.info()["precond_nnz"] == restated(name, level).nnz
    assert _same_bits(_factor(S), restated(name, level))
    S.close()


def test_every_width_class_is_hit(D, systems):
    """The factor cases above reach every width class of the device kernels: the class counts the device reports for them."""
    seen = {}
    for name, level in (("poisson2d_48", 1), ("poisson2d_48", 2), ("poisson3d_40", 2), ("quadtree", 3), ("quadtree_random", 3), ("delaunay_4000", 2)):
        assert (name, level) in FACTOR_CASES
        S = D.CsrSystem.from_any(systems[name], reorder=None)
        S.set_preconditioner(D.FSAI(level=level))
        seen[(name, level)] = [S.fsai_info()["columns_by_width"][w] for w in R.WIDTH_CLASSES]
        S.close()
    for k, w in enumerate(R.WIDTH_CLASSES):
        assert any(c[k] > 0 for c in seen.values()), f"no case has a column in the class m <= {w}"
    assert seen[("delaunay_4000", 2)][4] > 0
    assert seen[("quadtree", 3)][4] == 2 and seen[("quadtree_random", 3)][4] == 27


def test_reordered_handle_gives_the_same_bits(D, systems, restated):
    S = D.CsrSystem.from_any(systems["quadtree_random"], reorder="rcm")
    assert S.info()["reordered"]
    S.set_preconditioner(D.FSAI(level=2))
    Lr = restated("quadtree_random", 2)
    assert _same_bits(_factor(S), Lr)
    # ... and the permuted copies the SpMVs of a reordered handle read are those of LLtMultiply(restated L)
    T = D.CsrSystem.from_any(systems["quadtree_random"], reorder="rcm")
    T.set_preconditioner(D.LLtMultiply(Lr))
    b = _dev(O.rhs(S.n, 0))
    res, ref = S.solve(b), T.solve(b)
    assert res.status == 0 and res.iterations == ref.iterations and np.array_equal(res.res_history, ref.res_history)
    assert np.array_equal(res.x.cpu().numpy(), ref.x.cpu().numpy())
    S.close()
    T.close()


def test_explicit_pattern(D, systems, restated):
    A = systems["poisson2d_48"]
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(pattern=sp.tril(A).tocsr()))
    assert S.fsai_info()["level"] == 0
    assert _same_bits(_factor(S), restated("poisson2d_48", 1))
    P = O.learned_like_factor_preconditioning(A)                       # the pattern the reference's network emits
    P.sort_indices()
    counts, max_m = R.width_class_counts(A, pattern=P)
    assert max_m <= R.MAX_M
    S.set_preconditioner(D.FSAI(pattern=P))
    info = S.fsai_info()
    assert info["max_m"] == max_m and [info["columns_by_width"][w] for w in R.WIDTH_CLASSES] == counts and not info["pattern_reused"]
    Lr = R.fsai(A, pattern=P)
    assert np.array_equal(Lr.indptr, P.indptr) and np.array_equal(Lr.indices, P.indices)
    assert _same_bits(_factor(S), Lr)
    S.set_preconditioner(D.FSAI(pattern=(P.indptr, P.indices)))      # the same key again: only values
    assert S.fsai_info()["pattern_reused"] and _same_bits(_factor(S), Lr)
    S.close()


@pytest.mark.parametrize("name,level", [("poisson2d_48", 2), ("quadtree", 2)])
def test_apply(D, systems, restated, name, level):
    A, Lr = systems[name], restated(name, level)
    r = O.rhs(A.shape[0], 3)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(level=level))
    T = D.CsrSystem.from_any(A, reorder=None)
    T.set_preconditioner(D.LLtMultiply(Lr))
    z = S.precond_apply(_dev(r)).cpu().numpy()
    assert np.array_equal(z, T.precond_apply(_dev(r)).cpu().numpy())
    zr = Lr @ (Lr.T @ r)
    np.testing.assert_allclose(z, zr, rtol=1e-11, atol=1e-12 * np.abs(zr).max())
    S.close()
    T.close()


@pytest.mark.parametrize("name,level,form", [("poisson2d_48", 1, "small"), ("poisson2d_48", 2, "small"), ("poisson2d_256", 1, "chip"),
                                             ("poisson2d_256", 2, "chip"), ("quadtree", 2, "launches")])
def test_solve(D, systems, restated, name, level, form):
    A, Lr = systems[name], restated(name, level)
    n = A.shape[0]
    b = O.rhs(n, 0)
    S = D.CsrSystem.from_any(A, reorder=None)
    T = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    jac = S.solve(_dev(b))
    S.set_preconditioner(D.FSAI(level=level))
    T.set_preconditioner(D.LLtMultiply(Lr))
    if form == "chip":                                              # the one-launch whole-chip form takes the factor as it is
        assert S.chip_info()["chip_eligible"] and T.chip_info()["chip_eligible"]
    res, ref = S.solve(_dev(b)), T.solve(_dev(b))
    print(f"{name} level {level}: jacobi {jac.iterations}, fsai {res.iterations}")
    assert res.status == 0 and res.iterations == ref.iterations
    assert np.array_equal(res.res_history, ref.res_history) and np.array_equal(res.x.cpu().numpy(), ref.x.cpu().numpy())
    assert res.iterations < jac.iterations
    _, it, hist, _ = CO.pcg(A, b, "llt_multiply", L=Lr)
    assert abs(res.iterations - it) <= 0.06 * it + 2
    m = min(len(hist), len(res.res_history), 30)
    np.testing.assert_allclose(res.res_history[:m], hist[:m], rtol=1e-9)
    r_true = b - A @ res.x.cpu().numpy()
    assert np.dot(r_true, r_true) / np.dot(b, b) < 1.5e-8
    S.close()
    T.close()


def test_update_values_reuses_the_symbolic_phase(D, systems):
    A = systems["quadtree"]
    n = A.shape[0]
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.FSAI(level=2))
    assert not S.fsai_info()["pattern_reused"]
    d = 1.0 + 0.5 * np.sin(np.arange(n) * (2 * np.pi / n))          # a smooth positive diagonal scaling D A D
    A2 = _csr(sp.diags(d) @ A @ sp.diags(d))
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    S.update_values(A2.data)
    with pytest.raises(D._lib.DpcgError) as e:
        S.fsai_info()                                               # the factor went with the old values
    assert e.value.status == D._lib.ERR_STATE
    S.set_preconditioner(D.FSAI(level=2))
    assert S.fsai_info()["pattern_reused"]
    assert _same_bits(_factor(S), R.fsai(A2, level=2))
    S.set_preconditioner(D.FSAI(level=1))                           # another key: the symbolic phase runs again
    assert not S.fsai_info()["pattern_reused"]
    assert _same_bits(_factor(S), R.fsai(A2, level=1))
    S.close()


def _jacobi_history(S, b):
    return S.solve(_dev(b)).res_history


def test_errors_leave_the_previous_preconditioner(D, systems):
    # a negative diagonal entry: the local Cholesky of that column fails
    A = systems["poisson2d_48"].copy().tolil()
    A[100, 100] = -4.0
    A = _csr(A.tocsr())
    b = O.rhs(A.shape[0], 0)
    with pytest.raises(R.FsaiError) as re:
        R.fsai(A, level=1)
    S = D.CsrSystem.from_any(systems["poisson2d_48"], reorder=None)
    S.update_values(A.data)
    S.set_preconditioner(D.Jacobi(1.0 / np.abs(A.diagonal())))
    before = _jacobi_history(S, b)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(level=1))
    assert e.value.status == D._lib.ERR_PIVOT and f"column {re.value.column}" in str(e.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI and np.array_equal(_jacobi_history(S, b), before)
    S.close()
    # one column wider than the cap: a Delaunay mesh at level 2 (m = 74), and a dense row of 80 entries at level 1
    A = systems["delaunay_20000"]
    with pytest.raises(R.FsaiError) as re:
        R.fsai(A, level=2)
    assert re.value.kind == "width"
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    b = O.rhs(A.shape[0], 0)
    before = _jacobi_history(S, b)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(level=2))
    assert e.value.status == D._lib.ERR_INVALID and f"column {re.value.column} " in str(e.value) and "m = 74" in str(e.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI and np.array_equal(_jacobi_history(S, b), before)
    with pytest.raises(D._lib.DpcgError) as e:                      # level 4: refused by the C entry point
        D._lib.check(D._lib.lib().dpcg_set_precond_fsai(S._h, 4, None))
    assert e.value.status == D._lib.ERR_INVALID
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    S.close()
    B = sp.lil_matrix(O.poisson2d(20))
    B[0, 1:80] = -0.01
    B[1:80, 0] = -0.01
    B = _csr(B.tocsr())
    assert B.indptr[1] - B.indptr[0] == 80
    S = D.CsrSystem.from_any(B, reorder=None)
    S.set_preconditioner(D.Jacobi())
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(level=1))
    assert e.value.status == D._lib.ERR_INVALID and "column 0 " in str(e.value) and "m = 80" in str(e.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    # a pattern without a diagonal
    P = sp.tril(B).tolil()
    P[5, 5] = 0
    P = P.tocsr()
    P.eliminate_zeros()
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.FSAI(pattern=P))
    assert e.value.status == D._lib.ERR_INVALID and S.info()["precond"] == D._lib.PRECOND_JACOBI
    S.close()


def test_spectrum_bounds(D, systems):
    S = D.CsrSystem.from_any(systems["poisson2d_48"], reorder=None)
    S.set_preconditioner(D.Jacobi())
    kj = S.spectrum_bounds().kappa
    S.set_preconditioner(D.FSAI(level=1))
    k1 = S.spectrum_bounds().kappa
    print(f"kappa: jacobi {kj}, fsai(1) {k1}")
    assert np.isfinite(k1) and k1 < kj
    S.close()


def test_harness_rows(D, systems, tmp_path):
    from deeppreconditioning_amd.benchmark_suite import BenchmarkSuite, ListDataSet
    mats = [_csr(O.poisson2d(24)), _csr(O.poisson2d(32))]
    rhs = [O.rhs(m.shape[0], i) for i, m in enumerate(mats)]
    suite = BenchmarkSuite(ListDataSet(mats, rhs), None, techniques=("jacobi", "sparse_approximate_inverse"), results_directory=tmp_path)
    suite.run()
    suite.dump_csv()
    with open(tmp_path / "table.csv") as f:
        rows = {r["technique"]: r for r in csv.DictReader(f)}
    assert set(rows) == {"jacobi", "sparse_approximate_inverse"}
    assert float(rows["jacobi"]["successes"]) == 100 and float(rows["sparse_approximate_inverse"]["successes"]) == 100
    assert float(rows["sparse_approximate_inverse"]["iterations"]) < float(rows["jacobi"]["iterations"])
