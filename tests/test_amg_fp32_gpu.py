"""SmoothedAggregation(precision="fp32") (dpcg_set_precond_amg_precision): the device cycle against tests/amg_fp32_restatement.py
fed the device's own hierarchy, the hierarchy's bits against the fp64 attach, solves, determinism, re-attach, switching the
precision on one handle, batches, the spectrum, refusals and the harness row.

The apply test's bound: with e = |vcycle32 - vcycle| / |vcycle| (what the roundings do to the cycle, restatement against
restatement) and d = |M_dev x - vcycle32| / |vcycle32|, d <= e / 10.  A rounding that is misplaced, forgotten or applied twice
shows at the size of e itself; other fp64 summation orders can only flip single fp32 roundings."""

import csv
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amg_fp32_restatement as R32
import amg_restatement as R
import amg_smoother_restatement as SR
from deeppreconditioning_amd import meshes
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (smoother, constructor arguments): what the fp32 cycle takes
CASES = [("jacobi", dict(sweeps=1)), ("jacobi", dict(sweeps=2)), ("chebyshev", dict(degree=2))]
SYSTEMS = ["poisson2d_97", "poisson3d_24", "quadtree_random"]
REORDER = {"poisson2d_97": None, "poisson3d_24": None, "quadtree_random": "rcm"}


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def systems():
    """Built once.  9 409 rows (a multiple of no block size), 13 824 rows, and the smallest refined quadtree mesh (hanging nodes)
    that still gives three levels at max_coarse=100 (980 rows), numbered at random."""
    return {
        "poisson2d_97": _csr(O.poisson2d(97)),
        "poisson3d_24": _csr(O.poisson3d(24)),
        "quadtree_random": _csr(meshes.quadtree_fv_laplacian(30, 0, numbering="random")),
    }


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def _attach(D, A, reorder=None, **kw):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.SmoothedAggregation(**kw))
    return S


def _device(S, A, smoother, degree=2, eig_ratio=30.0):
    """The device's hierarchy as an R.Hierarchy and the smoothers the restatements must apply to replay its cycle."""
    info = S.amg_hierarchy()
    H = R.Hierarchy()
    Al = _csr(A)
    for l in range(info.levels - 1):
        lev = info.level(l)
        H.levels.append(R.Level(Al, 1.0 / Al.diagonal(), lev.aggregates, lev.P, info.omega[l]))
        Al = _csr(lev.A_next)
    H.levels.append(R.Level(Al, 1.0 / Al.diagonal()))
    H.coarse_inv = np.linalg.inv(Al.toarray())
    sm = SR.smoothers_for(H, smoother, degree=degree, eig_ratio=eig_ratio, rhos=info.rho, kinds=info.smoother)
    return info, H, sm


def _level_bits(S):
    info = S.amg_hierarchy()
    out = [info.rho, info.omega]
    for l in range(info.levels - 1):
        lev = info.level(l)
        out += [lev.aggregates, lev.P.indptr, lev.P.indices, lev.P.data, lev.A_next.indptr, lev.A_next.indices, lev.A_next.data]
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _apply(S, v):
    return S.precond_apply(torch.from_numpy(v).cuda()).cpu().numpy()


def _same_solve(a, b):
    return a.iterations == b.iterations and np.array_equal(a.res_history, b.res_history) and torch.equal(a.x, b.x)


# ---- 1. the apply -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother,kw", CASES)
@pytest.mark.parametrize("name", SYSTEMS)
def test_apply_equals_restatement(D, systems, name, smoother, kw):
    A = systems[name]
    S = _attach(D, A, reorder=REORDER[name], smoother=smoother, max_coarse=100, precision="fp32", **kw)
    assert S.reordered == (REORDER[name] is not None)
    info, H, sm = _device(S, A, smoother, degree=kw.get("degree", 2))
    assert info.levels >= 3 and info.precision == "fp32" and info.smoother == [smoother] * (info.levels - 1)
    nu = kw.get("sweeps", 1)
    x = np.random.default_rng(3).standard_normal(A.shape[0])
    ref64 = SR.vcycle(H, sm, x, nu)
    ref32 = R32.vcycle32(H, x, sm, nu)
    e = np.linalg.norm(ref32 - ref64) / np.linalg.norm(ref64)
    Mx = _apply(S, x)
    d = np.linalg.norm(Mx - ref32) / np.linalg.norm(ref32)
    print(f"fp32 apply {name} {smoother} {kw}: d = {d:.3e}  e = {e:.3e}")
    assert 0.0 < e <= 1e-5
    assert d <= e / 10
    assert np.array_equal(Mx, _apply(S, x))                      # two applies: the same bits


# ---- 2. the hierarchy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_hierarchy_untouched(D, systems, smoother):
    A = systems["poisson2d_97"]
    S64 = _attach(D, A, smoother=smoother, max_coarse=100)
    S32 = _attach(D, A, smoother=smoother, max_coarse=100, precision="fp32")
    h64, h32 = S64.amg_hierarchy(), S32.amg_hierarchy()
    assert (h64.precision, h32.precision) == ("fp64", "fp32")
    assert _same_bits(_level_bits(S64), _level_bits(S32))
    assert (h64.levels, h64.rows, h64.nnz, h64.p_nnz, h64.smoother, h64.chebyshev) == \
        (h32.levels, h32.rows, h32.nnz, h32.p_nnz, h32.smoother, h32.chebyshev)
    assert S64.info()["precond_nnz"] == S32.info()["precond_nnz"] == sum(h64.nnz) + 2 * sum(h64.p_nnz)
    assert h64.launches == h32.launches > 0
    lib = D._lib.lib()
    got = []
    for S in (S64, S32):
        n_launch, n_part = C.c_int(-1), C.c_int(-1)
        assert lib.dpcg_get_amg_launches(S._h, C.byref(n_launch), C.byref(n_part)) == 0
        got.append((n_launch.value, n_part.value))
    assert got[0] == got[1] and got[0][1] > 0
    assert S64.reduction_geometry() == S32.reduction_geometry()


# ---- 3. solves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_solve(D, systems, name, smoother):
    A = systems[name]
    b = O.rhs(A.shape[0], 0)
    bt = torch.from_numpy(b).cuda()
    S = _attach(D, A, reorder=REORDER[name], smoother=smoother, max_coarse=100, precision="fp32")
    r32 = S.solve(bt, rtol_sq=1e-8)
    assert r32.status == 0 and r32.res_history[-1] < 1e-8
    _, H, sm = _device(S, A, smoother)
    _, it, _, _ = O.preconditioned_conjugate_gradient(A, b, R32.VCycle32(H, sm, 1), rtol=1e-8)
    t32 = S.solve(bt, rtol_sq=1e-20, max_iter=200)
    S.set_preconditioner(D.SmoothedAggregation(smoother=smoother, max_coarse=100))
    assert S.amg_hierarchy().precision == "fp64"
    r64 = S.solve(bt, rtol_sq=1e-8)
    t64 = S.solve(bt, rtol_sq=1e-20, max_iter=200)
    res32 = np.linalg.norm(b - A @ t32.x.cpu().numpy())
    res64 = np.linalg.norm(b - A @ t64.x.cpu().numpy())
    print(f"fp32 solve {name} {smoother}: iterations fp32 {r32.iterations}, fp64 {r64.iterations}, restated fp32 {it}; "
          f"|b - A x| at rtol_sq=1e-20: fp32 {res32:.3e} ({t32.iterations} it), fp64 {res64:.3e} ({t64.iterations} it)")
    assert abs(r32.iterations - it) <= 2, (r32.iterations, it)
    assert abs(r32.iterations - r64.iterations) <= 1, (r32.iterations, r64.iterations)
    assert res32 <= 10 * res64, (res32, res64)                   # the preconditioner's precision does not limit the accuracy


# ---- 4. determinism and plumbing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_determinism_graph_and_reattach(D, systems, smoother):
    A = systems["poisson2d_97"]
    kw = dict(smoother=smoother, max_coarse=100, precision="fp32")
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S1, S2 = _attach(D, A, **kw), _attach(D, A, **kw)
    r1, r2 = S1.solve(b), S1.solve(b)
    assert _same_solve(r1, r2)
    rn = S2.solve(b, flags=D._lib.NO_GRAPH)
    assert _same_solve(rn, r1)
    # update_values(2 A) and a re-attach: the structures are kept as for fp64, the fp32 copies are made from the new values
    S64 = _attach(D, A, smoother=smoother, max_coarse=100)
    A2 = _csr(2.0 * A)
    for S, k in ((S1, kw), (S64, dict(kw, precision="fp64"))):
        S.update_values(A2.data)
        S.set_preconditioner(D.SmoothedAggregation(**k))
    h, h64 = S1.amg_hierarchy(), S64.amg_hierarchy()
    assert h.reused_levels == h64.reused_levels >= 1 and h.precision == "fp32"
    F = _attach(D, A2, **kw)
    assert F.amg_hierarchy().reused_levels == 0
    assert _same_bits(_level_bits(S1), _level_bits(F))
    assert _same_solve(S1.solve(b), F.solve(b))
    # a parked fp64 hierarchy re-attached as fp32 (and the other way round): the hierarchy is taken over, the copies are rebuilt
    S64.update_values(A.data)
    S64.set_preconditioner(D.SmoothedAggregation(**kw))
    assert S64.amg_hierarchy().reused_levels == h64.reused_levels and S64.amg_hierarchy().precision == "fp32"
    assert _same_solve(S64.solve(b), r1)


def test_switching_the_precision_on_one_handle(D, systems):
    A = systems["poisson2d_97"]
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    fresh = {p: _attach(D, A, max_coarse=100, precision=p).solve(b) for p in ("fp32", "fp64")}
    assert not torch.equal(fresh["fp32"].x, fresh["fp64"].x)       # (the two cycles are different operators)
    S = D.CsrSystem.from_any(A, reorder=None)
    for p in ("fp32", "fp64", "fp32"):
        S.set_preconditioner(D.SmoothedAggregation(max_coarse=100, precision=p))
        assert S.amg_hierarchy().precision == p
        assert _same_solve(S.solve(b), fresh[p]), p


def test_batch_mixes_fp32_amg_with_other_handles(D, systems):
    from deeppreconditioning_amd.batch import solve_batch
    mats = [systems["poisson2d_97"], O.poisson2d(64), systems["poisson3d_24"]]
    sys_ = [D.CsrSystem.from_any(m, reorder=None) for m in mats]
    sys_[0].set_preconditioner(D.SmoothedAggregation(max_coarse=100, precision="fp32"))
    sys_[1].set_preconditioner(D.Jacobi())
    sys_[2].set_preconditioner(D.SmoothedAggregation(smoother="chebyshev", max_coarse=100, precision="fp32"))
    rhs = [torch.from_numpy(O.rhs(m.shape[0], 0)).cuda() for m in mats]
    out = solve_batch(sys_, rhs, rtol_sq=1e-8)
    for s, b, r in zip(sys_, rhs, out):
        single = s.solve(b, rtol_sq=1e-8)
        assert r.status == 0 and r.iterations == single.iterations
        assert r.final_res == pytest.approx(single.final_res, rel=1e-10)
        assert torch.linalg.norm(r.x - single.x) <= 1e-8 * torch.linalg.norm(single.x)


def test_spectrum_bounds(D, systems):
    A = systems["poisson2d_97"]
    S = _attach(D, A, max_coarse=100, precision="fp32")
    sb32 = S.spectrum_bounds(rtol=1e-4)
    S.set_preconditioner(D.SmoothedAggregation(max_coarse=100))
    sb64 = S.spectrum_bounds(rtol=1e-4)
    print(f"fp32 spectrum: kappa fp32 {sb32.kappa:.6f}, fp64 {sb64.kappa:.6f}")
    assert sb32.lambda_min > 0
    assert abs(sb32.kappa - sb64.kappa) <= 1e-3 * sb64.kappa


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(D, systems):
    A = systems["poisson2d_97"]
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    lib = D._lib.lib()
    S = _attach(D, A, max_coarse=100, precision="fp32")
    before = S.solve(b, rtol_sq=1e-8)
    for smoother, precision in ((D._lib.AMG_GAUSS_SEIDEL, D._lib.AMG_FP32), (D._lib.AMG_JACOBI, 2), (D._lib.AMG_CHEBYSHEV, -1)):
        st = lib.dpcg_set_precond_amg_precision(S._h, 0.0, 10, 100, 1, 0, smoother, 2, 30.0, precision, None)
        assert st == D._lib.ERR_INVALID
        assert b"precision" in lib.dpcg_last_error()
    assert S.amg_hierarchy().precision == "fp32"
    assert _same_solve(S.solve(b, rtol_sq=1e-8), before)
    # DPCG_AMG_FP64 through the new entry point is dpcg_set_precond_amg_smoothed
    assert lib.dpcg_set_precond_amg_precision(S._h, 0.0, 10, 100, 1, 0, D._lib.AMG_GAUSS_SEIDEL, 2, 30.0, D._lib.AMG_FP64, None) == 0
    via_new = S.solve(b, rtol_sq=1e-8)
    assert lib.dpcg_set_precond_amg_smoothed(S._h, 0.0, 10, 100, 1, 0, D._lib.AMG_GAUSS_SEIDEL, 2, 30.0, None) == 0
    assert _same_solve(S.solve(b, rtol_sq=1e-8), via_new)
    J = D.CsrSystem.from_any(A, reorder=None)
    J.set_preconditioner(D.Jacobi())
    p = C.c_int(7)
    assert lib.dpcg_get_amg_precision(J._h, C.byref(p)) == D._lib.ERR_STATE and p.value == 7
    assert lib.dpcg_get_amg_launches(J._h, C.byref(p), None) == D._lib.ERR_STATE and p.value == 7


# ---- 6. one larger run --------------------------------------------------------------------------------------------------------
def test_poisson3d_64_and_the_harness_row(D, tmp_path):
    A = _csr(O.poisson3d(64))
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = _attach(D, A, precision="fp32")
    r32 = S.solve(b, rtol_sq=1e-8)
    S.set_preconditioner(D.SmoothedAggregation())
    r64 = S.solve(b, rtol_sq=1e-8)
    assert r32.status == 0 and r64.status == 0
    assert abs(r32.iterations - r64.iterations) <= 1, (r32.iterations, r64.iterations)
    from deeppreconditioning_amd.benchmark_suite import COMPARABILITY, BenchmarkSuite, ListDataSet
    P = O.poisson2d(24)
    names = ("jacobi", "algebraic_multigrid", "algebraic_multigrid_fp32")
    suite = BenchmarkSuite(ListDataSet([P], [O.rhs(P.shape[0], 0)]), None, techniques=names, results_directory=tmp_path)
    suite.run()
    suite.dump_csv()
    with (tmp_path / "table.csv").open() as f:
        rows = {r[0]: r for r in csv.reader(f)}
    assert "algebraic_multigrid_fp32" in rows
    assert COMPARABILITY["algebraic_multigrid_fp32"].startswith("not in the reference")
    assert suite.kappas["algebraic_multigrid_fp32"][0] < suite.kappas["jacobi"][0]
    assert suite.kappas["algebraic_multigrid_fp32"][0] == pytest.approx(suite.kappas["algebraic_multigrid"][0], rel=1e-3)
