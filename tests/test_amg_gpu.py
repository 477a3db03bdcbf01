"""SmoothedAggregation (dpcg_set_precond_amg): the device hierarchy against the numpy restatement (tests/amg_restatement.py), the
V-cycle apply, determinism, same-pattern reuse, solves, errors and the harness's `algebraic_multigrid` row."""

import csv

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amg_restatement as R
from deeppreconditioning_amd import meshes
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def systems():
    """Built once per module (the mesh generators take seconds)."""
    return {
        "poisson2d_256": O.poisson2d(256),
        "poisson3d_64": O.poisson3d(64),
        "quadtree_foam": meshes.quadtree_fv_laplacian(300, 5),
        "quadtree_random": meshes.quadtree_fv_laplacian(300, 5, numbering="random"),
        "delaunay": meshes.delaunay_laplacian(100000, 3),
    }


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def _rel(X, Y):
    return sp.linalg.norm(X - Y) / sp.linalg.norm(Y)


def _device_hierarchy(D, S, A):
    """The device's hierarchy as an R.Hierarchy (its A_l, P_l, omega_l; the coarsest level inverted here)."""
    info = S.amg_hierarchy()
    H = R.Hierarchy()
    Al = _csr(A)
    levels = []
    for l in range(info.levels - 1):
        lev = info.level(l)
        levels.append((lev, Al))
        H.levels.append(R.Level(Al, 1.0 / Al.diagonal(), lev.aggregates, lev.P, info.omega[l]))
        Al = _csr(lev.A_next)
    H.levels.append(R.Level(Al, 1.0 / Al.diagonal()))
    H.coarse_inv = np.linalg.inv(Al.toarray())
    return info, H, levels


def _attach(D, A, reorder=None, **kw):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.SmoothedAggregation(**kw))
    return S


@pytest.mark.parametrize("name", ["poisson2d_256", "poisson3d_64", "quadtree_foam", "quadtree_random", "delaunay", "reordered"])
def test_hierarchy_equals_restatement(D, systems, name):
    A = _csr(systems["quadtree_random" if name == "reordered" else name])
    S = _attach(D, A, reorder="rcm" if name == "reordered" else None)
    if name == "reordered":
        assert S.reordered
    info, H, levels = _device_hierarchy(D, S, A)
    assert info.levels >= 3 and info.rows[0] == A.shape[0] and info.rows[-1] <= 500
    assert S.info()["precond"] == D._lib.PRECOND_AMG
    assert S.info()["precond_nnz"] == sum(info.nnz) + 2 * sum(info.p_nnz)
    assert 1.0 < info.operator_complexity < 3.0 and 1.0 < info.grid_complexity < 2.0
    for l, (lev, Al) in enumerate(levels):
        Sg = R.strength(Al)
        agg = R.aggregate(Al, Sg, R.mis2(Sg, 0))                   # the rules applied to the device's A_l (caller numbering)
        assert np.array_equal(lev.aggregates, agg), f"level {l}: aggregates differ"
        w = info.omega[l]
        assert w == pytest.approx((4.0 / 3.0) / info.rho[l], rel=1e-15)
        T = R.tentative(agg)
        P = (T - sp.diags(w / Al.diagonal()) @ (Al @ T)).tocsr()
        assert _rel(lev.P, P) <= 1e-12, f"level {l}: P"
        assert _rel(lev.A_next, P.T @ (Al @ P)) <= 1e-12, f"level {l}: A_(l+1)"
        if Al.shape[0] <= 70000:
            lam = R.lambda_max_dinv_a(Al)
            assert lam <= info.rho[l] <= 1.05 * lam, (l, lam, info.rho[l])


def test_apply_equals_restatement_and_is_spd(D, systems):
    for A, reorder in ((systems["poisson2d_256"], None), (systems["quadtree_random"], "rcm")):
        A = _csr(A)
        S = _attach(D, A, reorder=reorder)
        _, H, _ = _device_hierarchy(D, S, A)
        rng = np.random.default_rng(3)
        x, y = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
        Mx = S.precond_apply(torch.from_numpy(x).cuda()).cpu().numpy()
        My = S.precond_apply(torch.from_numpy(y).cuda()).cpu().numpy()
        ref = R.vcycle(H, x)
        assert np.linalg.norm(Mx - ref) <= 1e-12 * np.linalg.norm(ref)
        assert abs(Mx @ y - x @ My) <= 1e-12 * np.linalg.norm(Mx) * np.linalg.norm(y)
    S = _attach(D, systems["poisson2d_256"])
    sb = S.spectrum_bounds(max_steps=200, rtol=1e-4)
    assert sb.lambda_min > 0 and sb.kappa < 10


def _level_bits(S):
    info = S.amg_hierarchy()
    out = [info.rho, info.omega]
    for l in range(info.levels - 1):
        lev = info.level(l)
        out += [lev.aggregates, lev.P.indptr, lev.P.indices, lev.P.data, lev.A_next.indptr, lev.A_next.indices, lev.A_next.data]
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_determinism_graph_and_reuse(D, systems):
    A = _csr(systems["quadtree_foam"])
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S1, S2 = _attach(D, A), _attach(D, A)
    assert _same_bits(_level_bits(S1), _level_bits(S2))
    r1, r2 = S1.solve(b), S1.solve(b)
    assert r1.iterations == r2.iterations and np.array_equal(r1.res_history, r2.res_history)
    assert torch.equal(r1.x, r2.x)
    rn = S2.solve(b, flags=D._lib.NO_GRAPH)
    assert rn.iterations == r1.iterations and np.array_equal(rn.res_history, r1.res_history) and torch.equal(rn.x, r1.x)
    assert S1.amg_hierarchy().reused_levels == 0 and S2.amg_hierarchy().reused_levels == 0


def _reattach_equals_fresh(D, S, A_new, b, reorder):
    S.update_values(A_new.data)
    S.set_preconditioner(D.SmoothedAggregation())
    F = _attach(D, A_new, reorder=reorder)                      # a fresh handle in the same numbering
    assert _same_bits(_level_bits(S), _level_bits(F))
    ru, rf = S.solve(b), F.solve(b)
    assert ru.iterations == rf.iterations and np.array_equal(ru.res_history, rf.res_history) and torch.equal(ru.x, rf.x)
    return S.amg_hierarchy(), F.amg_hierarchy()


@pytest.mark.parametrize("reordered", [False, True])
def test_reattach_after_update_values(D, systems, reordered):
    A = _csr(systems["quadtree_foam"])
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    reorder = "rcm" if reordered else None
    S = _attach(D, A, reorder=reorder)
    assert S.reordered == reordered
    # 2 A: every |a_ij| comparison keeps its outcome (ties included), so every level keeps its aggregates and the re-attach takes the
    # structures of P, A P, P^T and A_(l+1) over from the parked hierarchy -- only the numeric passes run
    h, f = _reattach_equals_fresh(D, S, _csr(2.0 * A), b, reorder)
    assert h.reused_levels == h.levels - 1 and f.reused_levels == 0
    # d A d with a random d: the far rule reads the values, level 0's aggregates change -- the re-attach builds afresh
    rng = np.random.default_rng(11)
    d = sp.diags(rng.uniform(0.5, 2.0, A.shape[0]))
    A2 = _csr(d @ A @ d)
    assert np.array_equal(A2.indices, A.indices)
    h, _ = _reattach_equals_fresh(D, S, A2, b, reorder)
    assert h.reused_levels == 0


def test_single_aggregate_and_its_values_only_refresh(D):
    """A complete graph of 12 rows: one MIS(2) root, one aggregate -- P has a single column, P^T a single row, the coarsest level one
    row.  Built, then re-attached after update_values with another diagonal: the aggregate stays (every row is a neighbour of the
    root), so only values are computed again -- P^T's through the kept sort order -- while P = T - omega D^-1 A T changes row by row."""
    n = 12
    A = _csr(np.diag(n + 1.0 + np.arange(n)) - np.ones((n, n)))
    A2 = _csr(np.diag((n + 1.0 + np.arange(n)) * np.linspace(1.0, 2.0, n)) - np.ones((n, n)))
    assert np.array_equal(A2.indices, A.indices)
    S = _attach(D, A, max_coarse=4)
    x = np.random.default_rng(5).standard_normal(n)
    for M, fresh in ((A, None), (A2, lambda: _attach(D, A2, max_coarse=4))):
        if fresh is not None:
            S.update_values(M.data)
            S.set_preconditioner(D.SmoothedAggregation(max_coarse=4))
        info, H, levels = _device_hierarchy(D, S, M)
        assert info.levels == 2 and info.rows == [n, 1] and info.reused_levels == (0 if fresh is None else 1)
        lev, Al = levels[0]
        Sg = R.strength(Al)
        assert np.array_equal(lev.aggregates, R.aggregate(Al, Sg, R.mis2(Sg, 0))) and not lev.aggregates.any()
        P = (R.tentative(lev.aggregates) - sp.diags(info.omega[0] / Al.diagonal()) @ (Al @ R.tentative(lev.aggregates))).tocsr()
        assert lev.P.shape == (n, 1) and _rel(lev.P, P) <= 1e-12 and _rel(lev.A_next, P.T @ (Al @ P)) <= 1e-12
        ref = R.vcycle(H, x)                                       # (restricts with scipy's transpose of the device's P)
        Mx = S.precond_apply(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.linalg.norm(Mx - ref) <= 1e-12 * np.linalg.norm(ref)
        if fresh is not None:
            F = fresh()
            assert _same_bits(_level_bits(S), _level_bits(F))
            assert torch.equal(S.precond_apply(torch.from_numpy(x).cuda()), F.precond_apply(torch.from_numpy(x).cuda()))


def test_level_copies_refuse_a_rebuilt_hierarchy(D, systems):
    import ctypes as C
    S = _attach(D, systems["poisson2d_256"])
    snap = S.amg_hierarchy()
    S.set_preconditioner(D.SmoothedAggregation(max_coarse=600))     # 568 rows: level 2 becomes the coarsest
    now = S.amg_hierarchy()
    assert now.levels != snap.levels or now.rows != snap.rows
    with pytest.raises(RuntimeError):
        snap.level(0)
    assert now.level(0).aggregates.size == 65536
    # the C entry point checks the sizes the buffers were made for: nothing is written when they do not match
    sizes = np.array([snap.rows[0], snap.p_nnz[0] - 1, snap.rows[1], snap.nnz[1]], dtype=np.int64)
    tiny = np.zeros(1, dtype=np.int32)
    st = D._lib.lib().dpcg_get_amg_level(S._h, 0, sizes.ctypes.data_as(C.c_void_p), tiny.ctypes.data_as(C.c_void_p),
                                         None, None, None, None, None, None, None)
    assert st == D._lib.ERR_INVALID and tiny[0] == 0


@pytest.mark.parametrize("name", ["poisson2d_256", "poisson3d_64", "quadtree_foam", "quadtree_random", "delaunay"])
def test_solve_matches_restatement_pcg(D, systems, name):
    A = _csr(systems[name])
    b = O.rhs(A.shape[0], 0)
    S = _attach(D, A)
    res = S.solve(torch.from_numpy(b).cuda(), rtol_sq=1e-8)
    assert res.status == 0 and res.res_history[-1] < 1e-8
    _, H, _ = _device_hierarchy(D, S, A)
    _, it, _, _ = O.preconditioned_conjugate_gradient(A, b, R.VCycle(H), rtol=1e-8)
    assert abs(res.iterations - it) <= 2, (res.iterations, it)
    x = res.x.cpu().numpy()
    assert np.linalg.norm(b - A @ x) <= 1e-3 * np.linalg.norm(b)


def test_one_million_rows(D):
    A = meshes.quadtree_fv_laplacian(1000, 0)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A)
    S.set_preconditioner(D.Jacobi())
    rj = S.solve(b, rtol_sq=1e-8, max_iter=1024)
    S.set_preconditioner(D.SmoothedAggregation())
    ra = S.solve(b, rtol_sq=1e-8, max_iter=1024)
    assert rj.status == 1 and ra.status == 0 and ra.iterations < 1024, (rj.iterations, ra.iterations)
    A3 = O.poisson3d(100)
    S3 = _attach(D, A3, reorder="auto")
    r3 = S3.solve(torch.from_numpy(O.rhs(A3.shape[0], 0)).cuda(), rtol_sq=1e-8)
    assert r3.status == 0 and r3.iterations <= 40, r3.iterations


def test_batch_mixes_amg_with_other_handles(D, systems):
    from deeppreconditioning_amd.batch import solve_batch
    mats = [systems["poisson2d_256"], O.poisson2d(64), systems["quadtree_foam"]]
    sys_ = [D.CsrSystem.from_any(m, reorder=None) for m in mats]
    sys_[0].set_preconditioner(D.SmoothedAggregation())
    sys_[1].set_preconditioner(D.Jacobi())
    sys_[2].set_preconditioner(D.SmoothedAggregation(sweeps=2))
    rhs = [torch.from_numpy(O.rhs(m.shape[0], 0)).cuda() for m in mats]
    out = solve_batch(sys_, rhs, rtol_sq=1e-8)
    for s, b, r in zip(sys_, rhs, out):
        single = s.solve(b, rtol_sq=1e-8)
        assert r.status == 0 and r.iterations == single.iterations
        assert r.final_res == pytest.approx(single.final_res, rel=1e-10)


def test_errors_leave_the_handle_usable(D):
    A = _csr(O.poisson2d(64))
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    for bad in (0.0, -1.0):
        B = A.copy()
        B[5, 5] = bad
        B = _csr(B)
        S = D.CsrSystem.from_any(B, reorder=None)
        with pytest.raises(D._lib.DpcgError):
            S.set_preconditioner(D.SmoothedAggregation())
    S = D.CsrSystem.from_any(A, reorder=None)
    S2 = D.CsrSystem.from_any(_csr(O.poisson2d(100)), reorder=None)
    with pytest.raises(D._lib.DpcgError) as exc:
        S2.set_preconditioner(D.SmoothedAggregation(max_levels=1))       # 10 000 rows on the coarsest level
    assert exc.value.status == D._lib.ERR_INVALID and "level 0" in str(exc.value)
    S2.set_preconditioner(D.SmoothedAggregation())
    r = S2.solve(torch.from_numpy(O.rhs(10000, 0)).cuda(), rtol_sq=1e-8)
    assert r.status == 0
    S.set_preconditioner(D.SmoothedAggregation())
    assert S.solve(b, rtol_sq=1e-8).status == 0


def test_harness_row(D, tmp_path):
    from deeppreconditioning_amd.benchmark_suite import BenchmarkSuite, ListDataSet
    A = O.poisson2d(24)
    data = ListDataSet([A], [O.rhs(A.shape[0], 0)])
    suite = BenchmarkSuite(data, None, techniques=("vanilla", "jacobi", "algebraic_multigrid"), results_directory=tmp_path)
    suite.run()
    suite.dump_csv()
    with (tmp_path / "table.csv").open() as f:
        rows = {r[0]: r for r in csv.reader(f)}
    assert "algebraic_multigrid" in rows
    with (tmp_path / "comparability.csv").open() as f:
        comp = {r[0]: r[1] for r in csv.reader(f)}
    assert "smoothed_aggregation" in comp["algebraic_multigrid"]
    assert suite.kappas["algebraic_multigrid"][0] < suite.kappas["jacobi"][0]
