"""SmoothedAggregation(smoother="gauss_seidel" | "chebyshev") (dpcg_set_precond_amg_smoothed): the hierarchy does not depend on the
smoother, the device colourings, the cycle against tests/amg_smoother_restatement.py fed the device's levels, colours and rho,
symmetry, solves, determinism, reuse, the Jacobi fallback, errors, batches and the harness rows."""

import csv
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amg_restatement as R
import amg_smoother_restatement as SR
from deeppreconditioning_amd import meshes
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = [("gauss_seidel", dict(sweeps=1)), ("gauss_seidel", dict(sweeps=2)), ("chebyshev", dict(degree=2)),
         ("chebyshev", dict(degree=3))]


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def systems():
    return {
        "poisson2d_256": O.poisson2d(256),
        "quadtree_foam": meshes.quadtree_fv_laplacian(300, 5),
        "quadtree_random": meshes.quadtree_fv_laplacian(300, 5, numbering="random"),
    }


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def _attach(D, A, reorder=None, **kw):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.SmoothedAggregation(**kw))
    return S


def _device(D, S, A, smoother, degree=2, eig_ratio=30.0):
    """The device's hierarchy as an R.Hierarchy and the smoothers the restatement must apply to replay its cycle."""
    info = S.amg_hierarchy()
    H = R.Hierarchy()
    Al = _csr(A)
    colors = []
    for l in range(info.levels - 1):
        lev = info.level(l)
        H.levels.append(R.Level(Al, 1.0 / Al.diagonal(), lev.aggregates, lev.P, info.omega[l]))
        colors.append(lev.colors)
        Al = _csr(lev.A_next)
    H.levels.append(R.Level(Al, 1.0 / Al.diagonal()))
    H.coarse_inv = np.linalg.inv(Al.toarray())
    sm = SR.smoothers_for(H, smoother, degree=degree, eig_ratio=eig_ratio, rhos=info.rho, colorings=colors, kinds=info.smoother)
    return info, H, sm, colors


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


def test_hierarchy_does_not_depend_on_the_smoother(D, systems):
    A = _csr(systems["poisson2d_256"])
    bits = [_level_bits(_attach(D, A, smoother=s)) for s in ("jacobi", "gauss_seidel", "chebyshev")]
    assert _same_bits(bits[0], bits[1]) and _same_bits(bits[0], bits[2])


@pytest.mark.parametrize("reorder", [None, "rcm"])
def test_colourings_are_proper_and_deterministic(D, systems, reorder):
    A = _csr(systems["quadtree_random"])
    S1, S2 = _attach(D, A, reorder=reorder, smoother="gauss_seidel"), _attach(D, A, reorder=reorder, smoother="gauss_seidel")
    assert S1.reordered == (reorder is not None)
    info, H, _, colors = _device(D, S1, A, "gauss_seidel")
    assert info.smoother == ["gauss_seidel"] * (info.levels - 1) and info.chebyshev == [None] * (info.levels - 1)
    _, _, _, colors2 = _device(D, S2, A, "gauss_seidel")
    for l, (c, c2) in enumerate(zip(colors, colors2)):
        assert c.dtype == np.int32 and c.shape == (info.rows[l],)
        assert SR.is_proper(H.levels[l].A, c)                 # level 0 in the caller's numbering: proper on the caller's A
        assert info.colors[l] == int(c.max()) + 1 and np.array_equal(np.unique(c), np.arange(info.colors[l]))
        assert np.array_equal(c, c2)


@pytest.mark.parametrize("smoother,kw", CASES)
def test_apply_equals_restatement(D, systems, smoother, kw):
    for A, reorder in ((systems["poisson2d_256"], None), (systems["quadtree_random"], "rcm")):
        A = _csr(A)
        S = _attach(D, A, reorder=reorder, smoother=smoother, **kw)
        info, H, sm, _ = _device(D, S, A, smoother, degree=kw.get("degree", 2))
        assert info.smoother == [smoother] * (info.levels - 1)
        if smoother == "chebyshev":
            assert info.chebyshev == [(r / 30.0, r) for r in info.rho[:-1]] and info.colors == [0] * (info.levels - 1)
        rng = np.random.default_rng(3)
        x, y = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        Mx, My = _apply(S, x), _apply(S, y)
        ref = SR.vcycle(H, sm, x, kw.get("sweeps", 1))
        assert np.linalg.norm(Mx - ref) <= 1e-12 * np.linalg.norm(ref)
        assert abs(Mx @ y - x @ My) <= 1e-12 * np.linalg.norm(Mx) * np.linalg.norm(y)


@pytest.mark.parametrize("smoother", ["gauss_seidel", "chebyshev"])
def test_dense_operator_is_spd(D, smoother):
    A = _csr(O.poisson2d(40))
    S = _attach(D, A, smoother=smoother, max_coarse=50)
    assert S.amg_hierarchy().levels >= 3
    E = torch.eye(A.shape[0], dtype=torch.float64, device="cuda")
    M = torch.stack([S.precond_apply(E[:, i].contiguous()) for i in range(A.shape[0])], dim=1).cpu().numpy()
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0


@pytest.mark.parametrize("smoother", ["gauss_seidel", "chebyshev"])
def test_solve_matches_restatement_pcg(D, systems, smoother):
    for A in (O.poisson2d(128), systems["quadtree_foam"]):
        A = _csr(A)
        b = O.rhs(A.shape[0], 0)
        S = _attach(D, A, smoother=smoother)
        res = S.solve(torch.from_numpy(b).cuda(), rtol_sq=1e-8)
        assert res.status == 0 and res.res_history[-1] < 1e-8
        _, H, sm, _ = _device(D, S, A, smoother)
        _, it, _, _ = O.preconditioned_conjugate_gradient(A, b, SR.VCycle(H, sm, 1), rtol=1e-8)
        assert abs(res.iterations - it) <= 2, (res.iterations, it)
        assert np.linalg.norm(b - A @ res.x.cpu().numpy()) <= 1e-3 * np.linalg.norm(b)


@pytest.mark.parametrize("smoother", ["gauss_seidel", "chebyshev"])
def test_determinism_graph_and_reattach(D, systems, smoother):
    A = _csr(systems["quadtree_foam"])
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S1, S2 = _attach(D, A, smoother=smoother), _attach(D, A, smoother=smoother)
    v = O.rhs(A.shape[0], 1)
    assert np.array_equal(_apply(S1, v), _apply(S2, v))
    r1, r2 = S1.solve(b), S2.solve(b, flags=D._lib.NO_GRAPH)
    assert r1.iterations == r2.iterations and np.array_equal(r1.res_history, r2.res_history) and torch.equal(r1.x, r2.x)
    # update_values(2 A) and a re-attach: the structures (colourings included) are kept and the result is a fresh setup's
    c0 = [S1.amg_hierarchy().level(l).colors for l in range(S1.amg_hierarchy().levels - 1)]
    A2 = _csr(2.0 * A)
    S1.update_values(A2.data)
    S1.set_preconditioner(D.SmoothedAggregation(smoother=smoother))
    F = _attach(D, A2, smoother=smoother)
    h = S1.amg_hierarchy()
    assert h.reused_levels == h.levels - 1
    assert _same_bits(_level_bits(S1), _level_bits(F))
    assert np.array_equal(_apply(S1, v), _apply(F, v))
    ru, rf = S1.solve(b), F.solve(b)
    assert ru.iterations == rf.iterations and np.array_equal(ru.res_history, rf.res_history) and torch.equal(ru.x, rf.x)
    if smoother == "gauss_seidel":
        c1 = [h.level(l).colors for l in range(h.levels - 1)]
        assert all(np.array_equal(x, y) for x, y in zip(c0, c1))


def test_uncolourable_level_falls_back_to_jacobi(D):
    n = 80
    B = 101.0 * np.eye(n) - np.ones((n, n)) + np.eye(n)        # dense SPD block: 80 colours needed
    A = _csr(sp.block_diag([O.poisson2d(40), sp.csr_matrix(B)]))
    S = _attach(D, A, smoother="gauss_seidel", max_coarse=50)
    info, H, sm, colors = _device(D, S, A, "gauss_seidel")
    assert info.smoother[0] == "jacobi" and info.colors[0] == 0 and colors[0] is None
    assert "gauss_seidel" in info.smoother[1:]
    st = D._lib.lib().dpcg_get_amg_colors(S._h, 0, A.shape[0], np.zeros(A.shape[0], dtype=np.int32).ctypes.data_as(C.c_void_p), None)
    assert st == D._lib.ERR_STATE
    x = O.rhs(A.shape[0], 2)
    ref = SR.vcycle(H, sm, x, 1)
    assert np.linalg.norm(_apply(S, x) - ref) <= 1e-12 * np.linalg.norm(ref)
    r = S.solve(torch.from_numpy(O.rhs(A.shape[0], 0)).cuda(), rtol_sq=1e-8)
    assert r.status == 0


def test_argument_errors_leave_the_handle_usable(D):
    A = _csr(O.poisson2d(64))
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = _attach(D, A, smoother="gauss_seidel")
    before = S.solve(b, rtol_sq=1e-8)
    lib = D._lib.lib()
    for smoother, degree, ratio in ((3, 2, 30.0), (-1, 2, 30.0), (2, 0, 30.0), (2, 9, 30.0), (2, 2, 1.0), (2, 2, float("nan")),
                                    (2, 2, float("inf"))):
        st = lib.dpcg_set_precond_amg_smoothed(S._h, 0.0, 10, 500, 1, 0, smoother, degree, ratio, None)
        assert st == D._lib.ERR_INVALID
    after = S.solve(b, rtol_sq=1e-8)
    assert after.iterations == before.iterations and torch.equal(after.x, before.x)
    n = A.shape[0]
    buf = np.full(n + 1, -7, dtype=np.int32)
    assert lib.dpcg_get_amg_colors(S._h, 0, n + 1, buf.ctypes.data_as(C.c_void_p), None) == D._lib.ERR_INVALID
    assert lib.dpcg_get_amg_colors(S._h, 99, n, buf.ctypes.data_as(C.c_void_p), None) == D._lib.ERR_INVALID
    assert np.all(buf == -7)
    S.set_preconditioner(D.SmoothedAggregation())
    assert lib.dpcg_get_amg_colors(S._h, 0, n, buf.ctypes.data_as(C.c_void_p), None) == D._lib.ERR_STATE
    assert S.amg_hierarchy().smoother == ["jacobi"] * (S.amg_hierarchy().levels - 1)
    S.set_preconditioner(D.SmoothedAggregation(smoother="chebyshev", degree=4, eig_ratio=12.0))
    assert S.solve(b, rtol_sq=1e-8).status == 0


def test_batch_mixes_the_smoothers_with_other_handles(D, systems):
    from deeppreconditioning_amd.batch import solve_batch
    mats = [systems["poisson2d_256"], O.poisson2d(64), systems["quadtree_foam"]]
    sys_ = [D.CsrSystem.from_any(m, reorder=None) for m in mats]
    sys_[0].set_preconditioner(D.SmoothedAggregation(smoother="gauss_seidel"))
    sys_[1].set_preconditioner(D.Jacobi())
    sys_[2].set_preconditioner(D.SmoothedAggregation(smoother="chebyshev", sweeps=2))
    rhs = [torch.from_numpy(O.rhs(m.shape[0], 0)).cuda() for m in mats]
    out = solve_batch(sys_, rhs, rtol_sq=1e-8)
    for s, b, r in zip(sys_, rhs, out):
        single = s.solve(b, rtol_sq=1e-8)
        assert r.status == 0 and r.iterations == single.iterations
        assert r.final_res == pytest.approx(single.final_res, rel=1e-10)


def test_harness_rows(D, tmp_path):
    from deeppreconditioning_amd.benchmark_suite import BenchmarkSuite, ListDataSet
    A = O.poisson2d(24)
    names = ("jacobi", "algebraic_multigrid_gauss_seidel", "algebraic_multigrid_chebyshev")
    suite = BenchmarkSuite(ListDataSet([A], [O.rhs(A.shape[0], 0)]), None, techniques=names, results_directory=tmp_path)
    suite.run()
    suite.dump_csv()
    with (tmp_path / "table.csv").open() as f:
        rows = {r[0]: r for r in csv.reader(f)}
    for name in names[1:]:
        assert name in rows
        assert suite.kappas[name][0] < suite.kappas["jacobi"][0]


def test_one_million_rows(D):
    A = meshes.quadtree_fv_laplacian(1000, 0)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A)
    for smoother in ("gauss_seidel", "chebyshev"):
        S.set_preconditioner(D.SmoothedAggregation(smoother=smoother))
        r = S.solve(b, rtol_sq=1e-8, max_iter=1024)
        assert r.status == 0 and r.iterations < 1024, (smoother, r.iterations)
