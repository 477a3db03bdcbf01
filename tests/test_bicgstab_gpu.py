"""BiCGStab on the device (dpcg_solve_bicgstab, dpcg_bicgstab.hip) against its numpy restatement (tests/bicgstab_restatement.py).

BiCGStab amplifies the difference between two summation orders exponentially in the update count (test_bicgstab_host.py has the
figures), so a whole history cannot be held to 1e-10 against an independent restatement.  The checks are split:
  short runs      max_iter = K = 6 (bicgstab_cases.K, measured on the CPU: the restatement's own spread between two summation orders
                  is <= 1e-12 there): history[0..K] and x within 1e-10 relative (x in the max norm) -- 100 x the verified spread;
  to the solution status, every history entry but the last >= rtol_sq, the count equal to the restatement's (both CPU summation
                  orders agree on it and stop with margins >= 1.2: asserted on the CPU), and the true residual of the returned x
                  within max(10 x the restatement's own gap, 1e-3 final_res) of final_res.
ILUT (item 3) runs on the non-symmetric 24x24_pe20 with three factors (bicgstab_cases.ILUT_VARIANTS): threshold 1e-3, where L keeps
1 104 and U 1 633 off-diagonal entries and U is not L^T; threshold 1e-2 (L = I, U upper triangular with 1 104); and ILUT's defaults,
which keep the diagonal only.  The device's factors are asserted to equal tests/ilut_restatement.py bit for bit in all three, which
is the evidence that the device ILUT assumes nothing about the symmetry of the values; the factors the restatement of BiCGStab applies
are the device's own (`lu_factors()`).  M = L U MULTIPLIED with the real factor approximates A, not its inverse: the restatement
diverges under both summation orders (test_bicgstab_host.py), so that pair has the short runs only -- which is where a wrong factor
order or slot shows -- and the multiplied form runs to the solution with the two weaker factors.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bicgstab_cases as C
import bicgstab_restatement as R

pytestmark = pytest.mark.gpu

K = C.K
SHORT_TOL = 1e-10


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def gpu(b):
    return torch.from_numpy(np.ascontiguousarray(b)).cuda()


def attach(D, name, pre, reorder=None):
    A = C.matrix(name)
    S = D.CsrSystem.from_any(A, reorder=reorder)
    if pre == "none":
        S.set_preconditioner(None)
    elif pre == "jacobi":
        S.set_preconditioner(D.Jacobi())
    elif pre == "csr":
        S.set_preconditioner(D.CsrPreconditioner(C.neumann_series_csr(A)))
    elif pre.startswith("ilut_"):
        mode, kw = C.ilut_mode(pre)
        S.set_preconditioner(D.ILUT(mode, **kw))
    else:
        raise KeyError(pre)
    return S


def device_m(S, name, pre):
    """the CPU M the restatement applies: for ILUT the DEVICE's factors (lu_factors), applied on the CPU"""
    if pre.startswith("ilut_"):
        Lf, Uf = S.lu_factors()
        Lr, Ur = C.ilut_factors(name, pre)
        n = Lf.shape[0]
        print(f"{pre}: the device's L holds {Lf.nnz - n} off-diagonal entries, its U {Uf.nnz - n}; max |U - L^T| {abs(Uf - Lf.T).max():.3g}")
        assert np.array_equal(Lf.toarray(), Lr.toarray()) and np.array_equal(Uf.toarray(), Ur.toarray()), \
            "the device ILUT of a non-symmetric matrix differs from the restatement"
        if pre in ("ilut_solve", "ilut_multiply"):       # the real L U: off-diagonal entries in both factors, U is not L^T
            assert Lf.nnz - n > 1000 and Uf.nnz - n > 1000 and abs(Uf - Lf.T).max() > 1.0
        return (C.lu_solve_apply if C.ilut_mode(pre)[0] == "solve" else C.lu_multiply_apply)(Lf, Uf)
    return C.precond_apply(name, pre)


def check_short(res, ref, what):
    assert res.iterations == ref["iterations"] and res.status == ref["status"], (what, res.iterations, res.status, ref["iterations"], ref["status"])
    assert len(res.res_history) == len(ref["history"])
    hs = R.rel_spread(res.res_history, ref["history"])
    xs = R.x_spread(res.x.cpu().numpy(), ref["x"]) if np.any(ref["x"]) else float(np.max(np.abs(res.x.cpu().numpy())))
    print(f"{what}: history within {hs:.2e}, x within {xs:.2e} of the restatement after {res.iterations} updates")
    assert hs <= SHORT_TOL and xs <= SHORT_TOL
    assert res.recurrence == "bicgstab" and res.final_res == res.res_history[-1]


def check_solution(D, name, pre, res, ref):
    A, b = C.matrix(name), C.rhs(name)
    assert res.status == D._lib.OK
    assert len(res.res_history) == res.iterations + 1
    assert np.all(res.res_history[:-1] >= C.RTOL_SQ) and res.res_history[-1] < C.RTOL_SQ
    assert res.iterations == ref["iterations"], (res.iterations, ref["iterations"])
    true = R.true_residual(A, b, res.x.cpu().numpy())
    gap_ref = abs(R.true_residual(A, b, ref["x"]) - ref["history"][-1])
    allowed = max(10.0 * gap_ref, 1e-3 * res.final_res)
    print(f"{name} {pre}: {res.iterations} updates; true residual {true:.6e}, final_res {res.final_res:.6e}, |difference| "
          f"{abs(true - res.final_res):.2e} <= {allowed:.2e} (10 x the restatement's gap {gap_ref:.2e} | 1e-3 final_res)")
    assert abs(true - res.final_res) <= allowed


# ---- 1. short runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", C.PRECONDS)
@pytest.mark.parametrize("name", C.SYSTEMS)
def test_short_runs_match_the_restatement(D, name, pre):
    S = attach(D, name, pre)
    b = C.rhs(name)
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=K)
    check_short(res, C.restated(name, pre, max_iter=K), f"{name} {pre}")


@pytest.mark.parametrize("pre", C.PRECONDS)
@pytest.mark.parametrize("name", ["23x23_pe2", "161x161_pe3"])
def test_short_runs_from_a_nonzero_x0_and_with_no_update(D, name, pre):
    A, b = C.matrix(name), C.rhs(name)
    x0 = np.random.default_rng(5).uniform(-1.0, 1.0, b.size)
    S = attach(D, name, pre)
    M = C.precond_apply(name, pre)
    res = S.solve_bicgstab(gpu(b), gpu(x0), rtol_sq=C.RTOL_SQ, max_iter=K)
    check_short(res, R.bicgstab(A, b, M, x0=x0, rtol_sq=C.RTOL_SQ, max_iter=K), f"{name} {pre} x0")
    res = S.solve_bicgstab(gpu(b), gpu(x0), rtol_sq=C.RTOL_SQ, max_iter=0)
    ref = R.bicgstab(A, b, M, x0=x0, rtol_sq=C.RTOL_SQ, max_iter=0)
    check_short(res, ref, f"{name} {pre} x0, max_iter = 0")
    assert res.status == D._lib.MAX_ITER and np.array_equal(res.x.cpu().numpy(), x0)
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=0)
    assert res.status == D._lib.MAX_ITER and res.iterations == 0 and res.res_history.tolist() == [1.0] and not res.x.any()


@pytest.mark.parametrize("pre", ["none", "jacobi"])
def test_one_and_two_rows(D, pre):
    for A, b in ((sp.csr_matrix(np.array([[3.0]])), np.array([2.0])),
                 (sp.csr_matrix(np.array([[4.0, -1.0], [-3.0, 5.0]])), np.array([1.0, -2.0]))):
        S = D.CsrSystem.from_any(A, reorder=None)
        S.set_preconditioner(D.Jacobi() if pre == "jacobi" else None)
        dinv = 1.0 / A.diagonal()
        ref = R.bicgstab(A, b, (lambda v: dinv * v) if pre == "jacobi" else None, rtol_sq=C.RTOL_SQ)
        res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ)
        assert res.status == D._lib.OK and res.iterations == ref["iterations"] <= 2
        np.testing.assert_allclose(res.x.cpu().numpy(), np.linalg.solve(A.toarray(), b), rtol=1e-6)
        np.testing.assert_allclose(res.x.cpu().numpy(), ref["x"], rtol=1e-10)


# ---- 2. to the solution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", C.PRECONDS)
@pytest.mark.parametrize("name", C.SOLVE_SYSTEMS)
def test_to_the_solution(D, name, pre):
    S = attach(D, name, pre)
    res = S.solve_bicgstab(gpu(C.rhs(name)), rtol_sq=C.RTOL_SQ, max_iter=C.MAX_ITER)
    check_solution(D, name, pre, res, C.restated(name, pre))


# ---- 3. ILUT, solved and multiplied ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", C.ILUT_PRECONDS)
def test_ilut_factors_as_m(D, pre):
    name = C.ILUT_SYSTEM
    A, b = C.matrix(name), C.rhs(name)
    S = attach(D, name, pre)
    M = device_m(S, name, pre)
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=K)
    check_short(res, R.bicgstab(A, b, M, rtol_sq=C.RTOL_SQ, max_iter=K), f"{name} {pre}")
    if pre in C.ILUT_DIVERGES:                            # (no run to the solution exists: see the head of this file)
        assert res.iterations == K and res.status == D._lib.MAX_ITER
        return
    res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=C.MAX_ITER)
    check_solution(D, name, pre, res, R.bicgstab(A, b, M, rtol_sq=C.RTOL_SQ, max_iter=C.MAX_ITER))


# ---- 4. a symmetric system; the handle's state is left alone -------------------------------------------------------------------
def test_a_symmetric_system_and_the_handle_afterwards(D):
    from oracle import oracle as O
    A = O.poisson2d(48)
    b = O.rhs(A.shape[0], 0)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    for flags in (0, D._lib.NO_SMALL):
        before = S.solve(gpu(b), flags=flags)
        res = S.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ)
        after = S.solve(gpu(b), flags=flags)
        assert res.status == D._lib.OK and res.res_history[-1] < C.RTOL_SQ <= res.res_history[-2]
        assert R.true_residual(A, b, res.x.cpu().numpy()) < 1.01 * C.RTOL_SQ
        assert before.iterations == after.iterations and before.status == after.status == D._lib.OK
        assert np.array_equal(before.res_history, after.res_history) and torch.equal(before.x, after.x)
        assert after.recurrence == "standard"


# ---- 5. a reordered handle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["jacobi", "csr"])
def test_a_reordered_handle_gives_the_same_iterate(D, pre):
    name = "64x64_pe5"
    b = C.rhs(name)
    plain = attach(D, name, pre).solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=K)
    Sr = attach(D, name, pre, reorder="rcm")
    assert Sr.reordered
    res = Sr.solve_bicgstab(gpu(b), rtol_sq=C.RTOL_SQ, max_iter=K)
    xs = R.x_spread(res.x.cpu().numpy(), plain.x.cpu().numpy())
    print(f"{name} {pre}: x of the reordered handle within {xs:.2e} of the unreordered one's after {K} updates")
    assert res.iterations == plain.iterations == K and xs <= SHORT_TOL
    check_short(res, C.restated(name, pre, max_iter=K), f"{name} {pre} rcm")


# ---- 6. / 7. reproducibility and the graph flag -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pre", [("161x161_pe3", "jacobi"), ("64x64_pe5", "csr"), ("24x24_pe20", "ilut_solve_u"),
                                      ("24x24_pe20", "ilut_multiply")])
def test_the_same_bits_twice(D, name, pre):
    S = attach(D, name, pre)
    b = gpu(C.rhs(name))
    one = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ, max_iter=60)
    two = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ, max_iter=60)
    assert two.iterations == one.iterations and two.status == one.status
    assert np.array_equal(two.res_history, one.res_history) and torch.equal(two.x, one.x)


def test_the_no_graph_flag_is_accepted(D):
    """The driver replays no graph, so `graph=False` (DPCG_NO_GRAPH) cannot take another path: this only holds the flag to being
    accepted and to changing nothing."""
    S = attach(D, "64x64_pe5", "jacobi")
    b = gpu(C.rhs("64x64_pe5"))
    one = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ, max_iter=60)
    two = S.solve_bicgstab(b, rtol_sq=C.RTOL_SQ, max_iter=60, graph=False)
    assert two.iterations == one.iterations and two.status == one.status
    assert np.array_equal(two.res_history, one.res_history) and torch.equal(two.x, one.x)


# ---- 8. the half-step exit and the cap ------------------------------------------------------------------------------------------
def test_half_step_exit_and_cap(D):
    d = np.linspace(1.0, 3.0, 9)
    bd = np.arange(1.0, 10.0)
    S = D.CsrSystem.from_any(sp.diags(d).tocsr(), reorder=None)
    S.set_preconditioner(D.Jacobi())
    res = S.solve_bicgstab(gpu(bd), rtol_sq=C.RTOL_SQ)
    # s = r - alpha v with v = d (dinv r) = r (1 + 2 u') and alpha = 1 + O(u): |s_i| <= 4 u |r_i|, u = 2^-53, so <s,s>/<b,b> <= 16 u^2
    assert res.status == D._lib.OK and res.iterations == 1 and res.res_history[0] == 1.0 and res.res_history[1] <= 16 * 2.0 ** -106
    np.testing.assert_allclose(res.x.cpu().numpy(), bd / d, rtol=1e-15)
    S = attach(D, "23x23_pe2", "none")
    res = S.solve_bicgstab(gpu(C.rhs("23x23_pe2")), rtol_sq=C.RTOL_SQ, max_iter=3)
    assert res.status == D._lib.MAX_ITER and res.iterations == 3 and len(res.res_history) == 4


# ---- 9. refusals and the breakdown ----------------------------------------------------------------------------------------------
def healthy(D):
    from oracle import oracle as O
    A = O.poisson2d(24)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    res = S.solve(gpu(O.rhs(A.shape[0], 0)))
    assert res.status == D._lib.OK


def refused(D, S, b, text, **kw):
    with pytest.raises(D._lib.DpcgError) as err:
        S.solve_bicgstab(gpu(b), **kw)
    assert err.value.status == D._lib.ERR_INVALID and "dpcg_solve_bicgstab" in str(err.value) and text in str(err.value), str(err.value)
    healthy(D)


def test_refusals(D):
    from deeppreconditioning_amd.operators import _dev_ptr, _stream
    from deeppreconditioning_amd.poisson import neumann_csr
    L = D._lib
    N = neumann_csr((8, 8))
    b = np.random.default_rng(0).uniform(-1.0, 1.0, 64)
    S = D.CsrSystem.from_any(N, reorder=None)
    S.set_nullspace("constant")
    refused(D, S, b - b.mean(), "null space")
    A = C.matrix("23x23_pe2")
    ba = C.rhs("23x23_pe2")
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_deflation(np.ones((A.shape[0], 1)))
    refused(D, S, ba, "deflation")

    class Twice:
        def __matmul__(self, v):
            return 2.0 * v
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.OperatorPreconditioner(Twice()))
    refused(D, S, ba, "callback")
    S = attach(D, "23x23_pe2", "jacobi")
    refused(D, S, ba, "max_iter", max_iter=-1)
    refused(D, S, ba, "finite", rtol_sq=float("nan"))
    refused(D, S, ba, "finite", atol_sq=float("inf"))
    bv, x = gpu(ba), torch.empty(ba.size, dtype=torch.float64, device="cuda")
    for flags in (L.INIT_CHECK_R, L.NO_SMALL, L.NO_GRAPH | L.SPMV_F32, L.SINGLE_REDUCTION):
        st = L.lib().dpcg_solve_bicgstab(S._h, _dev_ptr(bv), None, _dev_ptr(x), 1e-8, 0.0, 10, flags, _stream(), None, None, None, None)
        assert st == L.ERR_INVALID and b"DPCG_NO_GRAPH" in L.lib().dpcg_last_error()
        healthy(D)
    ok = S.solve_bicgstab(bv, rtol_sq=C.RTOL_SQ)           # the handle the refusals were made on is untouched
    assert ok.status == L.OK and ok.iterations == C.restated("23x23_pe2", "jacobi")["iterations"]


def test_a_zero_row_is_a_breakdown_not_a_fault(D):
    rowptr = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    col = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    val = torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
    S = D.CsrSystem(rowptr, col, val, 2, reorder=None)
    b = np.array([0.0, 1.0])
    for x0 in (None, np.array([0.0, 0.75])):            # (A x0 = 0 either way: r0 = b, v = A r0 = 0)
        res = S.solve_bicgstab(gpu(b), None if x0 is None else gpu(x0), rtol_sq=C.RTOL_SQ)
        ref = R.bicgstab(sp.csr_matrix(np.diag([1.0, 0.0])), b, x0=x0, rtol_sq=C.RTOL_SQ)
        assert ref["status"] == R.BREAKDOWN and ref["iterations"] == 0
        assert res.status == D._lib.BREAKDOWN and res.iterations == 0 and len(res.res_history) == 1
        x = res.x.cpu().numpy()
        assert np.all(np.isfinite(x)) and np.array_equal(x, np.zeros(2) if x0 is None else x0)
    healthy(D)
