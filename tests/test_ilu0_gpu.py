"""ILU(0) / DILU on the device (dpcg_set_precond_ilu0, dpcg_ilu0.hip) against the numpy restatement (tests/ilu0_restatement.py).

  factor      bit for bit the restatement of the matrix permuted by `precond_ordering()`, arrays laid out as the header says;
  ordering    a permutation, a proper colouring on these structurally symmetric patterns, the colour offsets are L's level sets;
  apply       U^-1 L^-1 r of the device's own factors by substitution on the CPU, mapped through the ordering, within 1e-12
              (test_ilu0_host.py: substitution is within 3.5e-16 of dense solves on these factors);
  BiCGStab    to the solution: status, true residual < 1.2 rtol_sq, the count of the restatement run with the device's own factors
              where that count is pinned (ilu0_cases.count_is_pinned: both CPU summation orders agree, margins >= 1.2 on both sides);
              short runs of K = 2 updates within SHORT_SPREAD x MARGIN = 1.2e-12 of the restatement;
  PCG         on symmetric matrices ILU(0) is IC(0) up to rounding: K = 6 history entries within PCG_SPREAD x MARGIN = 1.2e-13.
The tolerances are measured and reasoned in test_ilu0_host.py's header.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bicgstab_restatement as R
import ilu0_cases as C
import ilu0_restatement as I

pytestmark = pytest.mark.gpu

DEV_ORDER = {"caller": "caller", "colored": "multicolor"}       # the CPU's ordering tag -> the device's
SHORT_TOL = C.SHORT_SPREAD * C.MARGIN
PCG_TOL = C.PCG_SPREAD * C.MARGIN
APPLY_TOL = 1e-12


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def gpu(b):
    return torch.from_numpy(np.ascontiguousarray(b)).cuda()


def attach(D, A, variant="ilu0", order="caller", mode="solve", reorder=None):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.ILU0(mode, ordering=DEV_ORDER[order], variant=variant))
    return S


def arrays(M):
    return M.indptr, M.indices, M.data


def check_factor(S, A, variant, what):
    """the device's factors equal the restatement of A permuted by the device's ordering, array by array"""
    nc, perm = S.precond_ordering()
    n = A.shape[0]
    assert np.array_equal(np.sort(perm), np.arange(n)), "precond_ordering() is a permutation"
    Lf, Uf = S.lu_factors()
    Lr, Ur = I.FACTOR[variant](I.permuted(A, perm))
    for got, ref, tag in ((Lf, Lr, "L"), (Uf, Ur, "U")):
        for g, r, part in zip(arrays(got), arrays(ref), ("rowptr", "col", "val")):
            assert g.shape == r.shape and np.all(g == r), f"{what}: {tag}.{part} differs from the restatement"
    assert np.all(Lf.data[Lf.indptr[1:] - 1] == 1.0) and np.array_equal(Lf.indices[Lf.indptr[1:] - 1], np.arange(n))
    assert np.array_equal(Uf.indices[Uf.indptr[:-1]], np.arange(n))
    return nc, perm, Lf, Uf


def levels_of_lower(Lf):
    """level of every row of L from its strict lower pattern (rows ascending: a row's columns are finished)"""
    n = Lf.shape[0]
    lvl = np.zeros(n, dtype=np.int64)
    for i in range(n):
        cols = Lf.indices[Lf.indptr[i]:Lf.indptr[i + 1] - 1]
        if cols.size:
            lvl[i] = lvl[cols].max() + 1
    return lvl


def solve_by_levels(T, r):
    """T^-1 r for a triangular CSR T with few dependency levels, a level at a time (row sums in CSR order)"""
    n = T.shape[0]
    T = sp.csr_matrix(T, copy=True)
    T.sort_indices()
    d = T.diagonal()
    Soff = (T - sp.diags(d)).tocsr()
    Soff.eliminate_zeros()
    P = (Soff != 0).astype(np.int64).tocsr()
    lvl = np.zeros(n, dtype=np.int64)
    for _ in range(64):
        new = np.zeros(n, dtype=np.int64)
        has = np.diff(P.indptr) > 0
        new[has] = np.maximum.reduceat(lvl[P.indices], P.indptr[:-1][has]) + 1
        if np.array_equal(new, lvl):
            break
        lvl = new
    else:
        raise AssertionError("more than 64 levels: not a coloured factor")
    x = np.zeros(n)
    for l in range(lvl.max() + 1):
        rows = np.nonzero(lvl == l)[0]
        x[rows] = (r[rows] - Soff[rows] @ x) / d[rows]
    return x


def cpu_apply(Lf, Uf, perm, r, by_levels=False):
    if by_levels:
        z = np.empty_like(r)
        z[perm] = solve_by_levels(Uf, solve_by_levels(Lf, r[perm]))
        return z
    return I.lu_solve_apply(Lf, Uf, perm)(r)


# ---- 1. the factor, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,order", C.COMBOS)
def test_the_factor_equals_the_restatement_bit_for_bit(D, name, variant, order):
    A = C.matrix(name)
    S = attach(D, A, variant, order)
    nc, perm, Lf, Uf = check_factor(S, A, variant, f"{name} {variant} {order}")
    if order == "caller":
        assert nc == 0 and np.array_equal(perm, np.arange(A.shape[0]))
    assert S.info()["precond"] == D._lib.PRECOND_LU_SOLVE and S.info()["precond_nnz"] > 0


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("order", C.ORDERINGS)
def test_the_factor_on_a_reordered_handle(D, variant, order):
    A = C.matrix("24x24_pe20")
    S = attach(D, A, variant, order, reorder="rcm")
    assert S.reordered
    nc, perm, Lf, Uf = check_factor(S, A, variant, f"24x24_pe20 rcm {variant} {order}")
    if order == "caller":                                   # the caller's matrix: the bits of the handle that is not reordered
        assert np.array_equal(perm, np.arange(A.shape[0]))
    r = C.rhs("24x24_pe20", 3)
    z = S.precond_apply(gpu(r)).cpu().numpy()
    ref = cpu_apply(Lf, Uf, perm, r)
    assert np.max(np.abs(z - ref)) <= APPLY_TOL * np.max(np.abs(ref))


def test_multiply_mode_factors_the_callers_matrix(D):
    for name in ("7x5x3_pe3", "nine_9x7_pe3"):
        for variant in C.VARIANTS:
            A = C.matrix(name)
            S = attach(D, A, variant, "caller", mode="multiply")
            _, _, Lf, Uf = check_factor(S, A, variant, f"{name} {variant} multiply")
            assert S.info()["precond"] == D._lib.PRECOND_LU_MULTIPLY
            r = C.rhs(name, 3)
            z = S.precond_apply(gpu(r)).cpu().numpy()
            ref = Lf @ (Uf @ r)
            assert np.max(np.abs(z - ref)) <= APPLY_TOL * np.max(np.abs(ref))


# ---- 2. the ordering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SYSTEMS)
def test_the_multicolour_ordering_is_a_proper_colouring_and_its_offsets_are_the_levels_of_l(D, name):
    A = C.matrix(name)
    S = attach(D, A, "ilu0", "colored")
    nc, perm = S.precond_ordering()
    Lf, _ = S.lu_factors()
    lvl = levels_of_lower(Lf)
    assert np.all(np.diff(lvl) >= 0), "the factor's numbering lists the level sets of L one after the other"
    assert lvl.max() + 1 == nc == S.info()["levels_lower"], (lvl.max() + 1, nc, S.info())
    offsets = np.concatenate([[0], np.nonzero(np.diff(lvl))[0] + 1, [A.shape[0]]])
    colour = np.searchsorted(offsets, np.arange(A.shape[0]), side="right") - 1
    Ap = I.permuted(A, perm).tocoo()
    offd = Ap.row != Ap.col
    assert np.all(colour[Ap.row[offd]] != colour[Ap.col[offd]]), "no stored off-diagonal entry joins two rows of one colour"
    print(f"{name}: {nc} colours, sizes {np.diff(offsets).tolist()}")
    assert nc == 2 if name in C.GRIDS else nc >= 4


# ---- 3. the apply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,order", C.COMBOS)
def test_the_apply_is_two_substitutions_with_the_devices_factors(D, name, variant, order):
    A = C.matrix(name)
    S = attach(D, A, variant, order)
    _, perm = S.precond_ordering()
    Lf, Uf = S.lu_factors()
    r = C.rhs(name, 3)
    z = S.precond_apply(gpu(r)).cpu().numpy()
    ref = cpu_apply(Lf, Uf, perm, r)
    err = np.max(np.abs(z - ref)) / np.max(np.abs(ref))
    print(f"{name} {variant} {order}: apply within {err:.1e}")
    assert err <= APPLY_TOL
    again = S.precond_apply(gpu(r)).cpu().numpy()           # (the level-major vectors are left as the next apply needs them)
    assert np.array_equal(z, again)


def test_the_apply_at_48_cubed_takes_the_colour_sweeps(D):
    from deeppreconditioning_amd.poisson import convection_diffusion_csr
    A = convection_diffusion_csr((48, 48, 48), 3.0)
    S = attach(D, A, "ilu0", "colored")
    nc, perm = S.precond_ordering()
    Lf, Uf = S.lu_factors()
    info = S.info()
    assert nc == 2 and info["levels_lower"] == 2 and info["levels_upper"] == 2
    r = np.random.default_rng(3).uniform(-1.0, 1.0, A.shape[0])
    z = S.precond_apply(gpu(r)).cpu().numpy()
    ref = cpu_apply(Lf, Uf, perm, r, by_levels=True)
    err = np.max(np.abs(z - ref)) / np.max(np.abs(ref))
    print(f"48^3 multicolour: apply within {err:.1e}; residual of L U z = r on the CPU {np.max(np.abs(Lf @ (Uf @ z[perm]) - r[perm])):.1e}")
    assert err <= APPLY_TOL
    assert np.array_equal(z, S.precond_apply(gpu(r)).cpu().numpy())
    res = S.solve_bicgstab(gpu(r), rtol_sq=C.RTOL_SQ, max_iter=200)       # the in-loop apply (the sweeps sum nothing here, but run in a graph)
    assert res.status == D._lib.OK and R.true_residual(A, r, res.x.cpu().numpy()) < 1.2 * C.RTOL_SQ


# ---- 4. BiCGStab --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant,order", C.COMBOS)
def test_bicgstab_with_the_factor(D, name, variant, order):
    A, b = C.matrix(name), C.rhs(name)
    S = attach(D, A, variant, order)
    _, perm = S.precond_ordering()
    M = I.lu_solve_apply(*S.lu_factors(), perm)
    # short runs
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=C.K)
    ref = R.bicgstab(A, b, M, rtol_sq=C.RTOL_SQ, max_iter=C.K)
    assert res.iterations == ref["iterations"] and res.status == ref["status"] and len(res.res_history) == len(ref["history"])
    hs, xs = R.rel_spread(res.res_history, ref["history"]), R.x_spread(res.x.cpu().numpy(), ref["x"])
    print(f"{name} {variant} {order}: {C.K} updates: history within {hs:.2e}, x within {xs:.2e} of the restatement")
    assert hs <= SHORT_TOL and xs <= SHORT_TOL
    # to the solution
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=C.MAX_ITER)
    ref = R.bicgstab(A, b, M, rtol_sq=C.RTOL_SQ, max_iter=C.MAX_ITER)
    true = R.true_residual(A, b, res.x.cpu().numpy())
    pinned = C.count_is_pinned(name, variant, order) and ref["status"] == R.OK and C.margins_clear(ref["history"])
    print(f"{name} {variant} {order}: {res.iterations} updates (restated with the device's factors: {ref['iterations']}, "
          f"{'pinned' if pinned else 'not pinned'}); true residual {true:.3e}, final_res {res.final_res:.3e}")
    assert res.status == D._lib.OK and len(res.res_history) == res.iterations + 1
    assert np.all(res.res_history[:-1] >= C.RTOL_SQ) and res.res_history[-1] < C.RTOL_SQ
    assert true < 1.2 * C.RTOL_SQ
    if pinned:
        assert res.iterations == ref["iterations"]
        if order == "caller" or name in C.GRIDS:             # (the device's colours of a grid are the CPU's red and black)
            assert res.iterations == C.restated(name, variant, order)["iterations"]


def test_multicolour_ilu0_takes_fewer_updates_than_jacobi(D):
    name = "64x64_pe5"
    A, b = C.matrix(name), gpu(C.rhs(name))
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    jac = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ)
    S.set_preconditioner(D.ILU0("solve", ordering="multicolor"))
    ilu = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ)
    print(f"{name}: Jacobi {jac.iterations} updates, ILU(0) multicolour {ilu.iterations} (restated: 97 and 50)")
    assert jac.status == ilu.status == D._lib.OK and ilu.iterations < jac.iterations


# ---- 5. PCG on symmetric matrices ---------------------------------------------------------------------------------------------------
def symmetric_cases(D):
    from deeppreconditioning_amd.poisson import convection_diffusion_csr, poisson_csr
    rp, ci, v = (t.cpu().numpy() for t in poisson_csr(2, 32))
    yield "poisson_csr(2, 32)", sp.csr_matrix((v, ci, rp), shape=(1024, 1024))
    yield "24x24 peclet 0", convection_diffusion_csr((24, 24), 0.0)


def test_pcg_with_multicolour_ilu0_is_pcg_with_multicolour_ic0(D):
    for label, A in symmetric_cases(D):
        b = np.random.default_rng(0).uniform(-1.0, 1.0, A.shape[0])
        S = D.CsrSystem.from_any(A, reorder=None)
        S.set_preconditioner(D.ILU0("solve", ordering="multicolor"))
        full = S.solve(gpu(b), rtol_sq=C.RTOL_SQ)
        true = R.true_residual(A, b, full.x.cpu().numpy())
        assert full.status == D._lib.OK and full.res_history[-1] < C.RTOL_SQ and true < 1.2 * C.RTOL_SQ
        lu = S.solve(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=C.PCG_K)
        S.set_preconditioner(D.IC0("solve", ordering="multicolor"))
        ic = S.solve(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=C.PCG_K)
        s = R.rel_spread(lu.res_history[:C.PCG_K + 1], ic.res_history[:C.PCG_K + 1])
        print(f"{label}: PCG with ILU(0) converges in {full.iterations} updates (true residual {true:.3e}); its first {C.PCG_K} history "
              f"entries within {s:.1e} of IC(0)'s")
        assert len(lu.res_history) == len(ic.res_history) == C.PCG_K + 1 and s <= PCG_TOL


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def refuse(D, S, dinv, call, status, text):
    dinv = np.asarray(dinv, dtype=np.float64)
    S.set_preconditioner(D.Jacobi(dinv))
    with pytest.raises(D._lib.DpcgError) as exc:
        call()
    assert exc.value.status == status and text in str(exc.value), str(exc.value)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    r = np.arange(1.0, S.n + 1.0)
    assert np.array_equal(S.precond_apply(gpu(r)).cpu().numpy(), dinv * r), "the previous preconditioner stays attached"


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("order", ["caller", "multicolor"])
def test_bad_matrices_are_refused_and_jacobi_stays(D, variant, order):
    pc = lambda: D.ILU0("solve", ordering=order, variant=variant)
    A2 = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 1.0]]))              # a zero diagonal after elimination
    S = D.CsrSystem.from_any(A2, reorder=None)
    refuse(D, S, [1.0, 1.0], lambda: S.set_preconditioner(pc()), D._lib.ERR_PIVOT, "ILU(0): zero or non-finite pivot at row 1")
    res = S.solve_bicgstab(gpu(np.array([1.0, 1.0])), rtol_sq=C.RTOL_SQ)     # (b in the range of A: the half step of update 1 ends it)
    assert res.status == D._lib.OK and np.allclose(res.x.cpu().numpy().sum(), 1.0)
    A = C.matrix("7x5x3_pe3")
    dinv = 1.0 / A.diagonal()
    B = A.tolil()
    B[17, 17] = 0.0
    B = sp.csr_matrix(B)
    B.eliminate_zeros()                                                    # a missing diagonal
    S = D.CsrSystem.from_any(B, reorder=None)
    refuse(D, S, dinv, lambda: S.set_preconditioner(pc()), D._lib.ERR_PIVOT, "ILU(0): missing diagonal entry")
    N = A.copy()
    N.data[N.indptr[17]] = np.nan                                          # a NaN value
    S = D.CsrSystem.from_any(N, reorder=None)
    refuse(D, S, dinv, lambda: S.set_preconditioner(pc()), D._lib.ERR_PIVOT, "ILU(0): zero or non-finite pivot at row")


def test_bad_arguments_are_refused_and_jacobi_still_solves(D):
    Lb = D._lib
    name = "23x23_pe2"
    A, b = C.matrix(name), C.rhs(name)
    S = D.CsrSystem.from_any(A, reorder=None)
    dinv = 1.0 / A.diagonal()

    def raw(mode, variant, ordering):
        return lambda: Lb.check(Lb.lib().dpcg_set_precond_ilu0(S._h, mode, variant, ordering, None))
    refuse(D, S, dinv, raw(Lb.PRECOND_LU_MULTIPLY, Lb.ILU_ILU0, Lb.ORDER_MULTICOLOR), Lb.ERR_INVALID,
           "the multicolour ordering serves the triangular solves")
    refuse(D, S, dinv, raw(Lb.PRECOND_LU_SOLVE, 2, Lb.ORDER_CALLER), Lb.ERR_INVALID, "bad variant")
    refuse(D, S, dinv, raw(Lb.PRECOND_LU_SOLVE, Lb.ILU_DILU, 2), Lb.ERR_INVALID, "bad ordering")
    refuse(D, S, dinv, raw(Lb.PRECOND_LLT_SOLVE, Lb.ILU_ILU0, Lb.ORDER_CALLER), Lb.ERR_INVALID, "bad LU mode")
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ)
    assert res.status == Lb.OK and res.iterations == C.restated_jacobi(name)["iterations"]
    for kw in ({"mode": "apply"}, {"ordering": "rcm"}, {"variant": "ilu1"}, {"mode": "multiply", "ordering": "multicolor"}):
        with pytest.raises(ValueError):
            D.ILU0(**kw)
    with pytest.raises(TypeError):
        D.ILU0() @ gpu(b)


# ---- 7. the neighbours are unchanged --------------------------------------------------------------------------------------------------
def test_the_spectrum_of_a_nonsymmetric_m_is_refused_as_for_ilut(D):
    S = attach(D, C.matrix("23x23_pe2"), "ilu0", "colored")
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds()
    assert exc.value.status == D._lib.BREAKDOWN and "not symmetric" in str(exc.value)


def test_ilut_and_ic0_after_ilu0_give_the_bits_of_a_fresh_handle(D):
    from deeppreconditioning_amd.poisson import convection_diffusion_csr
    A = convection_diffusion_csr((24, 24), 0.0)                 # symmetric: IC(0) exists
    S = attach(D, A, "ilu0", "colored")
    S.set_preconditioner(D.ILUT("solve", add_fill_in=1, threshold=1e-3))
    F = D.CsrSystem.from_any(A, reorder=None)
    F.set_preconditioner(D.ILUT("solve", add_fill_in=1, threshold=1e-3))
    for X, Y in zip(S.lu_factors(), F.lu_factors()):
        assert all(np.array_equal(x, y) for x, y in zip(arrays(X), arrays(Y)))
    assert S.precond_ordering()[0] == 0 and np.array_equal(S.precond_ordering()[1], np.arange(A.shape[0]))
    r = gpu(np.random.default_rng(1).uniform(-1.0, 1.0, A.shape[0]))
    assert torch.equal(S.precond_apply(r), F.precond_apply(r))
    # the colouring cache: ILU(0) filled it, IC(0) reuses it, ILU(0) reuses it again
    S.set_preconditioner(D.ILU0("solve", ordering="multicolor"))
    p_lu = S.precond_ordering()
    S.set_preconditioner(D.IC0("solve", ordering="multicolor"))
    F.set_preconditioner(D.IC0("solve", ordering="multicolor"))
    assert all(np.array_equal(x, y) for x, y in zip(S.factor(), F.factor()))
    assert S.precond_ordering()[0] == F.precond_ordering()[0] == p_lu[0] and np.array_equal(S.precond_ordering()[1], F.precond_ordering()[1])
    assert np.array_equal(p_lu[1], F.precond_ordering()[1])
    assert torch.equal(S.precond_apply(r), F.precond_apply(r))
    S.set_preconditioner(D.ILU0("solve", ordering="multicolor", variant="dilu"))
    check_factor(S, A, "dilu", "after IC(0)")
    S.set_preconditioner(D.Jacobi())
    S.set_preconditioner(D.ILU0("solve", ordering="multicolor"))
    check_factor(S, A, "ilu0", "after Jacobi")


@pytest.mark.parametrize("order", C.ORDERINGS)
def test_update_values_drops_the_factor_and_the_next_attach_factors_the_new_values(D, order):
    from deeppreconditioning_amd.poisson import convection_diffusion_csr
    A, A2 = convection_diffusion_csr((23, 23), 2.0), convection_diffusion_csr((23, 23), 2.0, 1)
    assert np.array_equal(A.indices, A2.indices) and not np.array_equal(A.data, A2.data)
    S = attach(D, A, "ilu0", order)
    before = S.precond_ordering()[1]
    S.update_values(gpu(A2.data))
    with pytest.raises(D._lib.DpcgError):
        S.lu_factors()
    S.set_preconditioner(D.ILU0("solve", ordering=DEV_ORDER[order]))
    _, perm, _, _ = check_factor(S, A2, "ilu0", f"after update_values, {order}")
    assert np.array_equal(perm, before), "the colouring is the pattern's"
