"""The mixed-precision PCG kernels (dpcg_refine.hip) where the refinement loop cannot hide an error.

1.  Short runs: ONE inner solve of t = 1, 2, 3 updates (tests/refine_edge_cases.py) against the numpy restatement, per entry of x and
    of the inner history, within the measured tolerance: one fp32 ulp of ||x||_inf (twice the CPU spread is far below it) and 2^-22
    relative for a history entry.  The restatement with ONE matrix entry dropped lies >= 10 tolerances away at t = 2, 3
    (test_refine_edges_host.py), so a row kernel that drops, doubles or misreads an entry of any of these systems fails here.  The
    systems enter k_rf_spmv<2> .. <64>, odd and even row starts, rows of one entry, a row of 98 entries among short ones, stored
    zeros, and n = 1 .. 8 (no 16-byte group at all, and every n % 4).
2.  Stops and degenerate inputs, each against the restatement's prediction; every outer decision is >= 1.2 clear of its threshold
    (asserted on the CPU).  Update counts are compared only where the case forces them (a cap, zero updates, a breakdown).
3.  Invariants that need no tolerance: the same bits from call to call, from handle to handle, under DPCG_NO_GRAPH, on another
    stream, without the optional outputs, across preconditioner changes and new values on a reordered handle, and exact scaling
    under powers of two of A and b.

Observed on the MI355X (profiles/refine_edges.md): the largest distance of a short run from the restatement is 3.7e-9 ulp of x and
4.3e-16 relative of a history entry: the device's other summation order flips no fp32 rounding in these runs.
"""

import ctypes as C_

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_matrices as E
import refine_edge_cases as C
import refine_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def gpu(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def attach(D, A, pre, reorder=None):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.Jacobi() if pre == "jacobi" else None)
    return S


def last_error(D):
    return D._lib.lib().dpcg_last_error().decode(errors="replace")


def host(res):
    return res.x.cpu().numpy()


def same_bits(a, b):
    return (a.status == b.status and a.iterations == b.iterations and a.outer_steps == b.outer_steps and a.final_res == b.final_res
            and np.array_equal(a.res_history, b.res_history, equal_nan=True)
            and np.array_equal(a.outer_history, b.outer_history, equal_nan=True) and np.array_equal(host(a), host(b), equal_nan=True))


def residual_agrees(A, b, res):
    """final_res against an fp64 recomputation from the returned x, within R.residual_bound"""
    x = host(res)
    bb = float(b @ b)
    e = b - A @ x
    rr = float(e @ e)
    bound = R.residual_bound(A, b, x, rr)
    print(f"true <r,r> {rr:.6e}, the device's {res.final_res * bb:.6e}, bound {bound:.3e}")
    return abs(rr - res.final_res * bb) <= bound


# ---- 1. short runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pre,t", C.SHORT_CASES)
def test_short_run_matches_the_restatement_per_entry(D, name, pre, t):
    A, b = C.system(name)
    ref = C.short_run(name, pre, t)
    S = attach(D, A, pre)
    assert not S.reordered
    res = S.solve_refined(gpu(b), **C.short_kwargs(t))
    dx = C.x_distance(host(res), ref["x"], b)
    dh = C.hist_distance(res.res_history, ref["res_history"])
    print(f"OBSERVED | {name} | {pre} | {t} | {C.lanes_per_row(A)} | {dx:.3g} | {dh:.3g} |")
    assert (res.status, res.iterations, res.outer_steps) == (ref["status"], ref["iterations"], ref["outer_steps"])
    assert len(res.res_history) == res.iterations + 1 and len(res.outer_history) == res.outer_steps + 1
    assert res.res_history[0] == 1.0 and res.outer_history[0] == 1.0 and res.final_res == res.outer_history[-1]
    assert dx <= C.X_TOL_ULPS
    assert dh <= C.HIST_TOL
    assert residual_agrees(A, b, res)


# ---- 2. stops and degenerate inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.stop_cases()))
def test_stop_follows_the_restatement(D, case):
    L = D._lib
    ref = C.stop_restated(case)
    A, b, x0, pre, kw = C.stop_inputs(case)
    S = attach(D, A, pre)
    bt = gpu(b)
    x0t = None if x0 is None else gpu(x0)
    start = np.zeros_like(b) if x0 is None else x0
    with pytest.raises(L.DpcgError, match="max_outer"):              # leaves another text in dpcg_last_error
        S.solve_refined(bt, max_outer=0)
    res = S.solve_refined(bt, x0t, **kw)
    text = last_error(D)
    x = host(res)
    print(f"{case}: status {res.status}, {res.iterations} updates, {res.outer_steps} outer steps, outer history {res.outer_history} "
          f"(restatement {ref['status']}, {ref['iterations']}, {ref['outer_steps']}, {ref['outer_history']})")
    assert (res.status, res.outer_steps) == (ref["status"], ref["outer_steps"])
    assert len(res.res_history) == res.iterations + 1 and len(res.outer_history) == res.outer_steps + 1
    assert np.array_equal(np.isfinite(res.outer_history), np.isfinite(ref["outer_history"]))
    if case.startswith("atol_sq"):
        assert res.status == L.OK and res.final_res * float(b @ b) < kw["atol_sq"] and res.final_res > kw["rtol_sq"]
        assert residual_agrees(A, b, res)
    elif case.startswith("max_outer"):
        assert res.status == L.MAX_ITER and res.outer_steps == kw["max_outer"] and "stagnated" not in text
        assert np.all(np.diff(res.outer_history) < 0) and residual_agrees(A, b, res)
    elif case.startswith("cap at the end"):
        assert (res.status, res.iterations, res.outer_steps) == (L.MAX_ITER, kw["max_iter"], 1) and "stagnated" not in text
        assert residual_agrees(A, b, res)
    elif case.startswith("zero updates"):
        assert (res.status, res.iterations, res.outer_steps) == (L.MAX_ITER, 0, 1)
        assert "stagnated" in text
        assert np.array_equal(x, start) and len(res.res_history) == 1
        assert res.outer_history[1] == res.outer_history[0] and res.res_history[0] == res.outer_history[0]
    elif case.startswith("b = 0") or case.startswith("b with one NaN"):
        assert res.iterations == 0 and np.array_equal(x, start) and np.isnan(res.final_res)
    else:
        assert case == "fp32 rounds A to zero"
        assert (res.status, res.iterations, res.outer_steps) == (L.BREAKDOWN, 1, 1)
        assert np.array_equal(np.isfinite(x), np.isfinite(ref["x"])) and np.isnan(res.final_res)
        assert res.res_history[0] == 1.0 and np.isnan(res.res_history[1])
        S = attach(D, A, "jacobi")                                   # the same matrix under Jacobi is refused by name
        with pytest.raises(L.DpcgError, match="reciprocal diagonal entry 0 ") as e:
            S.solve_refined(bt)
        assert e.value.status == L.ERR_INVALID


def test_real_stagnation(D):
    """anisotropic2d(16, 1e-7), M = I, rtol_sq = 1e-30 (out of fp64's reach): three productive outer steps, then the fourth reduces
    <r,r> by less than 4 and the solve ends "stagnated".  Of the candidates scaled_rows(poisson2d(12), -4, 4) never has a productive
    step (the cap ends it), jumping((16, 16), 4, 1e8) stagnates at its first step with <r,r> grown by 1.1e4, and
    anisotropic2d(16, 1e-6) stagnates by a factor 1.18 only (and at another step under b (1 + 1e-16 u)); at 1e-7 the outer margins are
    >= 9.1, the stop itself 3.1, and every CPU perturbation ends at the same step (test_refine_edges_host.py)."""
    L = D._lib
    A, b, ref = C.stagnation_run(C.STAGNATION_CASE)
    S = attach(D, A, "identity")
    bt = gpu(b)
    S.solve_refined(bt)                                              # a converged call: no "stagnated" left over from it
    res = S.solve_refined(bt, rtol_sq=1e-30, max_iter=20000)
    print(f"{res.outer_steps} outer steps, {res.iterations} updates, outer history {res.outer_history} (restatement {ref['outer_steps']}, "
          f"{ref['iterations']}, {ref['outer_history']})")
    assert "stagnated" in last_error(D)
    assert (res.status, res.outer_steps) == (L.MAX_ITER, ref["outer_steps"]) and res.iterations < 20000
    assert np.isfinite(host(res)).all() and residual_agrees(A, b, res)
    assert res.outer_history[-1] >= 0.25 * res.outer_history[-2] and np.all(np.diff(res.outer_history[:-1]) < 0)


# ---- 3. invariants ------------------------------------------------------------------------------------------------------------------
INVARIANT_KW = dict(rtol_sq=1e-20, max_iter=2000)


@pytest.mark.parametrize("pre", C.PRES)
def test_bits_repeat(D, pre):
    A, b = C.system("hub(12, 97)")
    bt = gpu(b)
    S = attach(D, A, pre)
    first = S.solve_refined(bt, **INVARIANT_KW)
    assert first.status == D._lib.OK and first.outer_steps >= 2
    assert same_bits(S.solve_refined(bt, **INVARIANT_KW), first)                        # the same handle again
    assert same_bits(attach(D, A, pre).solve_refined(bt, **INVARIANT_KW), first)         # a fresh handle
    S2 = attach(D, A, pre)
    S2.solve_refined(gpu(np.random.default_rng(9).random(b.shape[0])), gpu(b), **INVARIANT_KW)
    assert same_bits(S2.solve_refined(bt, **INVARIANT_KW), first)                       # a handle that has solved something else


@pytest.mark.parametrize("pre", C.PRES)
def test_power_of_two_scaling_is_exact(D, pre):
    A, b = C.system(C.SCALING_SYSTEM)
    ref = C.scaling_restated(pre)
    base = attach(D, A, pre).solve_refined(gpu(b), **C.SCALING_KW)
    assert base.status == D._lib.OK and base.outer_steps == ref["outer_steps"]
    for k, m in C.SCALINGS:
        res = attach(D, A * 2.0 ** k, pre).solve_refined(gpu(b * 2.0 ** m), **C.SCALING_KW)
        assert (res.status, res.iterations, res.outer_steps) == (base.status, base.iterations, base.outer_steps), (k, m)
        assert np.array_equal(host(res), host(base) * 2.0 ** (m - k)), (k, m)
        assert np.array_equal(res.res_history, base.res_history) and np.array_equal(res.outer_history, base.outer_history), (k, m)


def raw_call(D, S, bt, flags, outputs, kw=INVARIANT_KW):
    """dpcg_solve_refined through ctypes: `flags`, and NULL for every optional output unless `outputs`"""
    L = D._lib
    x = torch.empty_like(bt)
    iters, outer, res, sec = C_.c_int(), C_.c_int(), C_.c_double(), C_.c_double()
    hist, outer_hist = np.full(kw["max_iter"] + 1, np.nan), np.full(17, np.nan)
    ptr = lambda a: a.ctypes.data_as(C_.c_void_p)
    opt = (C_.byref(iters), C_.byref(outer), C_.byref(res), C_.byref(sec), ptr(hist), ptr(outer_hist)) if outputs else (None,) * 6
    status = L.check(L.lib().dpcg_solve_refined(S._h, bt.data_ptr(), None, x.data_ptr(), kw["rtol_sq"], 0.0, kw["max_iter"], 1e-6, 16, flags,
                                                C_.c_void_p(torch.cuda.current_stream().cuda_stream), *opt))
    torch.cuda.synchronize()
    return status, x.cpu().numpy(), iters.value, outer.value, res.value, hist[: iters.value + 1], outer_hist[: outer.value + 1]


def test_no_graph_another_stream_and_absent_outputs_give_the_same_bits(D):
    L = D._lib
    A, b = C.system("banded_spd(203, 12, 2)")
    bt = gpu(b)
    S = attach(D, A, "jacobi")
    plain = S.solve_refined(bt, **INVARIANT_KW)
    assert plain.status == L.OK and plain.outer_steps >= 2
    status, x, iters, outer, fres, hist, outer_hist = raw_call(D, S, bt, L.NO_GRAPH, True)
    assert (status, iters, outer, fres) == (plain.status, plain.iterations, plain.outer_steps, plain.final_res)
    assert np.array_equal(x, host(plain)) and np.array_equal(hist, plain.res_history) and np.array_equal(outer_hist, plain.outer_history)
    status, x, *_ = raw_call(D, S, bt, 0, False)                                        # NULL iters, outer, final_res, seconds, histories
    assert status == plain.status and np.array_equal(x, host(plain))
    quiet = S.solve_refined(bt, want_history=False, **INVARIANT_KW)
    assert (quiet.status, quiet.iterations, quiet.outer_steps, quiet.final_res) == (plain.status, plain.iterations, plain.outer_steps, plain.final_res)
    assert torch.equal(quiet.x, plain.x) and len(quiet.res_history) == 0 and np.array_equal(quiet.outer_history, plain.outer_history)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = S.solve_refined(bt, **INVARIANT_KW)
    side.synchronize()
    assert same_bits(other, plain)


def test_preconditioner_changes_drop_the_fp32_copies(D):
    """identity -> Jacobi -> identity on one handle: each solve equals a fresh handle's bit for bit (a stale or missing dinv32 would
    give the bits of the other preconditioner, or fault)"""
    A, b = C.system("scaled_rows(banded_spd(130, 6, 3), -3, 3, 1)")
    bt = gpu(b)
    kw = dict(rtol_sq=1e-20, max_iter=3)                              # three updates: M decides every one of them
    fresh = {pre: attach(D, A, pre).solve_refined(bt, **kw) for pre in C.PRES}
    assert not np.array_equal(host(fresh["identity"]), host(fresh["jacobi"]))
    S = attach(D, A, "identity")
    for pre in ("identity", "jacobi", "identity", "jacobi"):
        S.set_preconditioner(D.Jacobi() if pre == "jacobi" else None)
        assert same_bits(S.solve_refined(bt, **kw), fresh[pre]), pre


@pytest.mark.parametrize("pre", C.PRES)
def test_update_values_on_a_reordered_handle(D, pre):
    A = E.poisson2d(20)
    perm = np.random.default_rng(3).permutation(A.shape[0])
    B = sp.csr_matrix(A[perm][:, perm])
    B.sort_indices()
    B.indices, B.indptr = B.indices.astype(np.int32), B.indptr.astype(np.int32)
    b = np.random.default_rng(1).random(A.shape[0])
    bt = gpu(b)
    S = attach(D, B, pre, reorder="rcm")
    assert S.reordered
    one = S.solve_refined(bt, **INVARIANT_KW)
    assert one.status == D._lib.OK
    S.update_values(2.0 * B.data)
    if pre == "jacobi":
        S.set_preconditioner(D.Jacobi())
    two = S.solve_refined(bt, **INVARIANT_KW)
    fresh = attach(D, 2.0 * B, pre, reorder="rcm").solve_refined(bt, **INVARIANT_KW)
    assert fresh.status == D._lib.OK and same_bits(two, fresh)
    assert residual_agrees(2.0 * B, b, two)
    assert np.linalg.norm(host(two) - 0.5 * host(one)) <= 1e-9 * np.linalg.norm(host(one))
