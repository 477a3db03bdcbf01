"""SmoothedAggregation beyond Poisson systems and default arguments: anisotropic, jumping-coefficient, non-M-matrix, identity-row,
disconnected, stored-zero, hub, tiny and scaled systems (tests/edge_matrices.py) with theta > 0, seed != 0 and a reordered handle;
the SpGEMM's long-row path on both sides of its LDS capacity; every smoother with several sweeps; a two-grid cycle against its
error propagator built from A, P and omega alone; the one-level hierarchy; the 4096-row limit of the coarsest level; solves."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amg_restatement as R
import amg_smoother_restatement as SR
import edge_matrices as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KSG_CAP = 1024                  # products of a Galerkin row sorted in LDS (k_spgemm); more go to global scratch
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


GENERATORS = {
    "aniso_1e-3": lambda: E.anisotropic2d(48, 1e-3),
    "aniso_1e-6": lambda: E.anisotropic2d(48, 1e-6),
    "jump2d": lambda: E.jumping((48, 48), 6),
    "jump3d": lambda: E.jumping((14, 14, 14), 3),
    "nine_point": lambda: E.nine_point_mixed(48),
    "bbt": lambda: E.random_bbt(2000),
    "identity_rows": lambda: E.boundary_identity(48),
    "three_components": E.three_components,
    "tiny_components": E.tiny_components,
    "stored_zeros": lambda: E.with_stored_zeros(E.poisson2d(48)),
    "scaled": lambda: E.scaled_rows(E.poisson2d(48)),
    "hub_1023": lambda: E.hub(40, 1023),
    "hub_1024": lambda: E.hub(40, 1024),
}


@pytest.fixture(scope="module")
def mats():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = GENERATORS[name]()
        return cache[name]
    return get


def _rel(X, Y):
    return sp.linalg.norm(X - Y) / sp.linalg.norm(Y)


def _attach(D, A, reorder=None, **kw):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.SmoothedAggregation(**kw))
    return S


def _levels(S, A):
    """[(AmgLevel l, A_l as scipy, omega_l)] for the smoothed levels, the coarsest A and the hierarchy info."""
    info = S.amg_hierarchy()
    out, Al = [], E.csr(A)
    for l in range(info.levels - 1):
        lev = info.level(l)
        out.append((lev, Al, info.omega[l]))
        Al = E.csr(lev.A_next)
    return info, out, Al


def _as_hierarchy(levels, Ac, sweeps=1):
    H = R.Hierarchy(sweeps=sweeps)
    for lev, Al, w in levels:
        H.levels.append(R.Level(Al, 1.0 / Al.diagonal(), lev.aggregates, lev.P, w))
    H.levels.append(R.Level(Ac, 1.0 / Ac.diagonal()))
    H.coarse_inv = np.linalg.inv(Ac.toarray())
    return H


def _check_levels(info, levels, Ac, theta, seed, max_coarse, max_levels=10):
    """Aggregates (integers) from the rules applied to the device's A_l; P = T - omega D^-1 A T and A_(l+1) = P^T A P by scipy."""
    for l, (lev, Al, w) in enumerate(levels):
        St = R.strength(Al, theta)
        roots = R.mis2(St, seed)
        agg = R.aggregate(Al, St, roots)
        assert np.array_equal(lev.aggregates, agg), f"level {l}: aggregates differ"
        assert info.rows[l + 1] == int(roots.sum())
        T = R.tentative(lev.aggregates)
        P = (T - sp.diags(w / Al.diagonal()) @ (Al @ T)).tocsr()
        assert _rel(lev.P, P) <= 1e-12, f"level {l}: P"
        assert _rel(lev.A_next, P.T @ (Al @ P)) <= 1e-12, f"level {l}: A_(l+1)"
    n = Ac.shape[0]
    assert n <= 4096
    if n > max_coarse and info.levels < max_levels:      # the build stopped because coarsening stalled: the rule says so too
        roots = R.mis2(R.strength(Ac, theta), seed)
        assert roots.sum() == 0 or roots.sum() > 0.9 * n


@pytest.mark.parametrize("reorder", [None, "rcm"])
@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("theta", [0.0, 0.08, 0.25])
@pytest.mark.parametrize("name", list(GENERATORS))
def test_hierarchy_equals_restatement_and_scipy(D, mats, name, theta, seed, reorder):
    A = mats(name)
    S = _attach(D, A, reorder=reorder, theta=theta, seed=seed, max_coarse=100)
    info, levels, Ac = _levels(S, A)
    assert info.rows[0] == A.shape[0]
    _check_levels(info, levels, Ac, theta, seed, 100)
    if theta == 0.0 and name not in ("tiny_components", "identity_rows", "three_components"):
        assert info.levels >= 2


def _galerkin_counts(levels):
    """Per level: the product counts of A T, A P and P^T (A P), from the device's A_l and P_l (A P's structure: the symbolic product)."""
    out = []
    for lev, Al, _ in levels:
        n = Al.shape[0]
        T = sp.csr_matrix((np.ones(n), lev.aggregates, np.arange(n + 1)), shape=(n, int(lev.aggregates.max()) + 1))
        AP = E.pattern_product(Al, lev.P)
        out.append((E.product_counts(Al, T), E.product_counts(Al, lev.P), E.product_counts(lev.P.T.tocsr(), AP)))
    return out


@pytest.mark.parametrize("k,long_at", [(1023, False), (1024, True)])
def test_spgemm_at_the_lds_capacity(D, mats, k, long_at):
    """The hub row of A T expands exactly k + 1 products: 1024 still sort in LDS, 1025 go to the global-scratch path."""
    A = mats(f"hub_{k}")
    S = _attach(D, A, reorder=None)
    info, levels, Ac = _levels(S, A)
    _check_levels(info, levels, Ac, 0.0, 0, 500)
    at, ap, ptap = _galerkin_counts(levels)[0]
    assert at.max() == k + 1 and at[-1] == k + 1
    assert (at.max() > KSG_CAP) == long_at
    assert ap.max() > KSG_CAP and ptap.max() > KSG_CAP     # A P and P^T (A P) take the long path at the hub either way


@pytest.mark.parametrize("name", ["hub_1023", "hub_1024"])
def test_spgemm_long_rows_far_past_the_capacity(D, mats, name):
    """P^T (A P) at the hub's aggregate expands ~1.9e5 products: a scratch segment of 2^18, sorted by one wave."""
    A = mats(name)
    S = _attach(D, A, reorder="rcm", theta=0.08, seed=7)
    info, levels, Ac = _levels(S, A)
    _check_levels(info, levels, Ac, 0.08, 7, 500)
    counts = _galerkin_counts(levels)
    biggest = max(int(c.max()) for trio in counts for c in trio)
    long_rows = sum(int((c > KSG_CAP).sum()) for trio in counts for c in trio)
    assert biggest > 128 * KSG_CAP and long_rows > 100, (biggest, long_rows)
    print(f"{name}: largest Galerkin row {biggest} products, {long_rows} rows on the long path")


@pytest.mark.parametrize("name,theta,seed,reorder", [("jump2d", 0.08, 7, "rcm"), ("aniso", 0.25, 0, None), ("aniso", 0.08, 7, "rcm")])
def test_theta_and_seed_at_1e5_rows(D, name, theta, seed, reorder):
    A = E.jumping((316, 316), 16) if name == "jump2d" else E.anisotropic2d(316, 1e-3)
    S = _attach(D, A, reorder=reorder, theta=theta, seed=seed)
    assert S.reordered == (reorder is not None)
    info, levels, Ac = _levels(S, A)
    assert info.levels >= 3
    _check_levels(info, levels, Ac, theta, seed, 500)
    assert R.strength(A, theta).nnz < R.strength(A, 0.0).nnz                  # the filter drops connections here


def test_scratch_beyond_2_31_entries_is_refused(D):
    """A hub of 1500 on a 316 x 316 grid: level 1's A P would need ~9.7e9 scratch entries for its long rows.  The int32 scan of
    the segment sizes wrapped to a small positive total and the sort ran outside the scratch; now the 64-bit total is checked
    and the setup returns DPCG_ERR_INVALID, keeping the preconditioner the handle had."""
    A = E.hub(316, 1500, seed=3)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    before = S.solve(b, rtol_sq=1e-8)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.set_preconditioner(D.SmoothedAggregation(theta=0.08, seed=7))
    assert exc.value.status == D._lib.ERR_INVALID and "2^31 scratch entries" in str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    after = S.solve(b, rtol_sq=1e-8)
    assert after.iterations == before.iterations and torch.equal(after.x, before.x)


def test_empty_strength_graph_stalls(D):
    """theta above every |a_ij| / sqrt(a_ii a_jj) (1/4 on the 5-point grid): every row is a root, coarsening stalls at level 0.
    1600 rows are solved densely (one level); 10 000 rows are refused, and the handle keeps the preconditioner it had."""
    A = E.poisson2d(40)
    S = _attach(D, A, theta=0.3)
    assert S.amg_hierarchy().levels == 1 and S.amg_hierarchy().rows[0] == 1600
    assert R.mis2(R.strength(A, 0.3), 0).all()
    B = E.poisson2d(100)
    b = torch.from_numpy(O.rhs(B.shape[0], 0)).cuda()
    S2 = D.CsrSystem.from_any(B, reorder=None)
    S2.set_preconditioner(D.Jacobi())
    before = S2.solve(b, rtol_sq=1e-8)
    with pytest.raises(D._lib.DpcgError) as exc:
        S2.set_preconditioner(D.SmoothedAggregation(theta=0.3))
    assert exc.value.status == D._lib.ERR_INVALID
    assert "level 0" in str(exc.value) and "10000 rows" in str(exc.value) and "4096" in str(exc.value)
    assert S2.info()["precond"] == D._lib.PRECOND_JACOBI
    after = S2.solve(b, rtol_sq=1e-8)
    assert after.iterations == before.iterations and np.array_equal(after.res_history, before.res_history)
    assert torch.equal(after.x, before.x)


APPLY_MATS = {
    "aniso": lambda: E.anisotropic2d(32, 1e-3),
    "jump2d": lambda: E.jumping((32, 32), 4),
    "nine_point": lambda: E.nine_point_mixed(32),
}
SMOOTHERS = [("jacobi", 1, 2), ("jacobi", 2, 2), ("jacobi", 3, 2), ("gauss_seidel", 1, 2), ("gauss_seidel", 2, 2),
             ("chebyshev", 1, 3), ("chebyshev", 2, 3), ("chebyshev", 2, 2)]


def _dense_m(S, n):
    E_ = torch.eye(n, dtype=torch.float64, device="cuda")
    return torch.stack([S.precond_apply(E_[:, i].contiguous()) for i in range(n)], dim=1).cpu().numpy()


@pytest.mark.parametrize("smoother,sweeps,degree", SMOOTHERS)
@pytest.mark.parametrize("name", list(APPLY_MATS))
def test_apply_equals_restatement_and_is_spd(D, name, smoother, sweeps, degree):
    A = APPLY_MATS[name]()
    n = A.shape[0]
    S = _attach(D, A, smoother=smoother, sweeps=sweeps, degree=degree, max_coarse=40)
    info, levels, Ac = _levels(S, A)
    assert info.levels >= 3 and info.smoother == [smoother] * (info.levels - 1)
    H = _as_hierarchy(levels, Ac)
    colors = [lev.colors for lev, _, _ in levels]
    sm = SR.smoothers_for(H, smoother, degree=degree, rhos=info.rho, colorings=colors, kinds=info.smoother)
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    Mx = S.precond_apply(torch.from_numpy(x).cuda()).cpu().numpy()
    My = S.precond_apply(torch.from_numpy(y).cuda()).cpu().numpy()
    ref = SR.vcycle(H, sm, x, sweeps)
    assert np.linalg.norm(Mx - ref) <= 1e-12 * np.linalg.norm(ref)
    assert abs(Mx @ y - x @ My) <= 1e-12 * np.linalg.norm(Mx) * np.linalg.norm(y)
    M = _dense_m(S, n)
    Mr = SR.dense_operator(H, sm, sweeps)
    assert np.linalg.norm(M - Mr) <= 1e-12 * np.linalg.norm(Mr)
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0


@pytest.mark.parametrize("sweeps", [1, 2, 3])
@pytest.mark.parametrize("name", ["aniso", "nine_point", "jump2d"])
def test_two_grid_equals_its_error_propagator(D, name, sweeps):
    """M = (I - E) A^-1 with E = S^nu (I - P A_c^-1 P^T A) S^nu, S = I - omega D^-1 A: from A, the device's P and omega alone."""
    A = APPLY_MATS[name]()
    n = A.shape[0]
    S = _attach(D, A, sweeps=sweeps, max_levels=2)
    info = S.amg_hierarchy()
    assert info.levels == 2
    P = info.level(0).P.toarray()
    Ad = A.toarray()
    w = info.omega[0]
    Sm = np.eye(n) - w * (1.0 / np.diag(Ad))[:, None] * Ad
    Ac = P.T @ Ad @ P
    C = np.eye(n) - P @ np.linalg.solve(Ac, P.T @ Ad)
    Snu = np.linalg.matrix_power(Sm, sweeps)
    Ep = Snu @ C @ Snu
    M = _dense_m(S, n)
    scale = np.linalg.norm(M, 2) * np.linalg.norm(Ad, 2)
    assert np.linalg.norm(M @ Ad - (np.eye(n) - Ep), 2) <= 1e-12 * scale


@pytest.mark.parametrize("name", ["tiny_1", "tiny_2", "tiny_3", "tiny_17", "poisson_400", "stall_1600"])
def test_one_level_is_the_dense_solve(D, name):
    if name.startswith("tiny"):
        A, kw = E.tiny(int(name.split("_")[1])), {}
    elif name == "poisson_400":
        A, kw = E.poisson2d(20), {}
    else:
        A, kw = E.jumping((40, 40), 5, 1e3), dict(theta=0.9)
    n = A.shape[0]
    S = _attach(D, A, **kw)
    info = S.amg_hierarchy()
    assert info.levels == 1 and info.rows == [n]
    Ad = A.toarray()
    kappa = np.linalg.cond(Ad)
    for seed in range(3):
        r = O.rhs(n, seed)
        z = S.precond_apply(torch.from_numpy(r).cuda()).cpu().numpy()
        want = np.linalg.solve(Ad, r)
        assert np.linalg.norm(z - want) <= 50 * EPS * kappa * np.linalg.norm(want)
    res = S.solve(torch.from_numpy(O.rhs(n, 0)).cuda(), rtol_sq=1e-20)
    assert res.status == 0 and 1 <= res.iterations <= 2, res.iterations


def _coarse_4096(extra):
    """block_diag(G, 2 I_m): G (the shifted 64 x 64 grid) coarsens to c aggregates, each of the m isolated rows is an aggregate of
    its own, so level 1 has c + m rows; m = 4096 - c + extra."""
    G = E.csr(E.poisson2d(64) + 2.0 * sp.identity(4096))
    c = int(R.mis2(R.strength(G), 0).sum())
    m = 4096 - c + extra
    return E.csr(sp.block_diag([G, 2.0 * sp.identity(m)])), c


def test_coarsest_level_of_4096_rows(D):
    A, _ = _coarse_4096(0)
    S = _attach(D, A, reorder=None, max_levels=2)
    info, levels, Ac = _levels(S, A)
    assert info.levels == 2 and info.rows[1] == 4096
    _check_levels(info, levels, Ac, 0.0, 0, 500, max_levels=2)
    H = _as_hierarchy(levels, Ac)
    x = O.rhs(A.shape[0], 4)
    ref = R.vcycle(H, x)
    got = S.precond_apply(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.linalg.norm(got - ref) <= 1e-12 * np.linalg.norm(ref)
    res = S.solve(torch.from_numpy(O.rhs(A.shape[0], 0)).cuda(), rtol_sq=1e-8)
    assert res.status == 0


def test_coarsest_level_of_4097_rows_is_refused(D):
    A, _ = _coarse_4096(1)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    before = S.solve(b, rtol_sq=1e-8)
    with pytest.raises(D._lib.DpcgError) as exc:          # (the isolated rows never coarsen: level 1 stalls at any max_levels)
        S.set_preconditioner(D.SmoothedAggregation(max_levels=2))
    assert exc.value.status == D._lib.ERR_INVALID and "level 1" in str(exc.value) and "4097 rows" in str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    after = S.solve(b, rtol_sq=1e-8)
    assert after.iterations == before.iterations and np.array_equal(after.res_history, before.res_history)
    assert torch.equal(after.x, before.x)
    S1 = D.CsrSystem.from_any(E.csr(sp.block_diag([E.poisson2d(64), sp.identity(1)])), reorder=None)
    with pytest.raises(D._lib.DpcgError) as exc:
        S1.set_preconditioner(D.SmoothedAggregation(max_levels=1))
    assert exc.value.status == D._lib.ERR_INVALID and "level 0" in str(exc.value) and "4097 rows" in str(exc.value)
    S1.set_preconditioner(D.SmoothedAggregation())
    assert S1.solve(torch.from_numpy(O.rhs(4097, 0)).cuda(), rtol_sq=1e-8).status == 0


SOLVE_MATS = {
    "aniso": lambda: E.anisotropic2d(64, 1e-3),
    "jump2d": lambda: E.jumping((64, 64), 8),
    "nine_point": lambda: E.nine_point_mixed(64),
}


@pytest.mark.parametrize("name", list(SOLVE_MATS))
def test_solve_matches_restatement_pcg(D, name):
    A = SOLVE_MATS[name]()
    b = O.rhs(A.shape[0], 0)
    rtol_sq = 1e-12
    S = _attach(D, A)
    res = S.solve(torch.from_numpy(b).cuda(), rtol_sq=rtol_sq)
    assert res.status == 0 and res.res_history[-1] < rtol_sq
    info, levels, Ac = _levels(S, A)
    _, it, hist, _ = O.preconditioned_conjugate_gradient(A, b, R.VCycle(_as_hierarchy(levels, Ac)), rtol=rtol_sq)
    # the same cycle: the histories agree while rounding has not yet been amplified; past ~200 iterations (the 1e6 jumps) the
    # two finite-precision CG runs drift apart by a few per cent
    np.testing.assert_allclose(res.res_history[:30], hist[:30], rtol=1e-6, atol=0)
    assert abs(res.iterations - it) <= max(2, 0.05 * it), (res.iterations, it)
    x = res.x.cpu().numpy()
    assert np.linalg.norm(b - A @ x) ** 2 <= 4 * rtol_sq * np.linalg.norm(b) ** 2
