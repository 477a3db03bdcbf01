"""Mixed-precision PCG on the device (dpcg_solve_refined, dpcg_refine.hip) against its numpy restatement (refine_restatement.py).

The true residual is recomputed here in fp64 from the returned x and compared with `final_res` within
|delta rr| <= 2 sqrt(rr) n eps || |A||x| + |b| ||_2 (R.residual_bound: computed, not chosen), and must meet the threshold within the same
bound.  Inner histories are NOT compared tightly: fp32 stores make them sensitive to the order of the fp64 sums.  Instead the device's
total update count must lie within COUNT_MARGIN of the restatement's.  That margin is measured (tools/refine_probe.py --cpu-spread,
profiles/refine_probe.md): over the 24 cases below the restatement's total moves by at most 0.65 % under b (1 + 1e-16 u),
b (1 + 1e-12 u) and dots summed back to front; twice that, 1.30 %, is allowed.  No case moved by more than 10 %, so none is excluded.

Count cases by the criterion of test_deflation_gpu.py are those where every outer AND every inner stop margin of the restatement is
>= 1.2.  The CPU classification found none: an inner solve tests once per update and these recurrences shrink <r,r> by a few per
cent per update, so some inner stop always lies within 1.2 of its target (the smallest inner margins are 1.002 .. 1.14).
COUNT_CASES is therefore empty and the test re-asserts that classification.  The number of OUTER steps, though, is decided by the
outer stops alone, and those are all clear of their thresholds (outer margins >= 3.4; the restatement's outer_steps does not move
under any of the perturbations of profiles/refine_probe.md).  So, deliberately stricter than that criterion, outer_steps must equal
the restatement's in every case whose outer margins are >= 1.2 -- OUTER_CASES, all 24 -- which is what catches a wrong target or
stagnation factor on the device.  The inner margins bear on the total count only, which has its measured margin above.
"""

import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import refine_cases as cases
import refine_restatement as R

pytestmark = pytest.mark.gpu

COUNT_MARGIN = 2 * 0.0065
COUNT_CASES = []
OUTER_CASES = list(cases.CASES)


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def gpu(b):
    return torch.from_numpy(np.ascontiguousarray(b)).cuda()


def attach(D, A, pre, reorder=None):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.Jacobi() if pre == "jacobi" else None)
    return S


def check_solution(D, A, b, res, rtol_sq):
    """the assertions every converged solve meets"""
    assert res.status == D._lib.OK
    assert res.final_res == res.outer_history[-1] and len(res.outer_history) == res.outer_steps + 1
    x = res.x.cpu().numpy()
    bb = float(b @ b)
    e = b - A @ x
    rr = float(e @ e)
    bound = R.residual_bound(A, b, x, rr)
    print(f"true <r,r> {rr:.6e}, the device's {res.final_res * bb:.6e}, bound {bound:.3e}; threshold {rtol_sq * bb:.6e}")
    assert abs(rr - res.final_res * bb) <= bound
    assert rr <= rtol_sq * bb + bound
    assert len(res.res_history) == res.iterations + 1 and res.res_history[0] == res.outer_history[0]
    assert np.all(np.isfinite(res.res_history))
    assert np.all(np.diff(res.outer_history) < 0)


@pytest.mark.parametrize("name,pre,rtol_sq", cases.CASES)
def test_against_the_restatement(D, name, pre, rtol_sq):
    A, b = cases.system(name)
    ref = cases.restated(name, pre, rtol_sq)
    S = attach(D, A, pre)
    res = S.solve_refined(gpu(b), rtol_sq=rtol_sq, max_iter=cases.MAX_ITER)
    margin = min(min(ref["outer_margins"]), min(ref["inner_margins"]))
    print(f"{name} {pre} {rtol_sq:g}: {res.iterations} updates in {res.outer_steps} outer steps (restatement {ref['iterations']} in "
          f"{ref['outer_steps']}, inner counts {ref['inner_counts']}), smallest stop margin {margin:.3f}")
    check_solution(D, A, b, res, rtol_sq)
    assert ref["status"] == R.OK
    assert ((name, pre, rtol_sq) in COUNT_CASES) == (margin >= 1.2), f"the classification of this case changed: margin {margin:.3f}"
    outer_margin = min(ref["outer_margins"])
    assert ((name, pre, rtol_sq) in OUTER_CASES) == (outer_margin >= 1.2), f"outer margin {outer_margin:.3f}"
    if (name, pre, rtol_sq) in OUTER_CASES:
        assert res.outer_steps == ref["outer_steps"]
    assert abs(res.iterations - ref["iterations"]) <= COUNT_MARGIN * ref["iterations"]


def test_reordered_handle(D):
    A, b = cases.system("poisson 40x40")
    perm = np.random.default_rng(3).permutation(A.shape[0])
    B = sp.csr_matrix(A[perm][:, perm])
    B.sort_indices()
    B.indices, B.indptr = B.indices.astype(np.int32), B.indptr.astype(np.int32)
    bp = b[perm]
    S = attach(D, B, "jacobi", reorder="rcm")
    assert S.reordered and S.permutation() is not None
    for rtol_sq in (1e-8, 1e-20):
        res = S.solve_refined(gpu(bp), rtol_sq=rtol_sq, max_iter=cases.MAX_ITER)
        check_solution(D, B, bp, res, rtol_sq)                                    # the caller's numbering
    x0 = np.random.default_rng(4).random(A.shape[0])
    res = S.solve_refined(gpu(bp), gpu(x0), rtol_sq=1e-20, max_iter=cases.MAX_ITER)
    check_solution(D, B, bp, res, 1e-20)


def test_x0_cap_and_converged_start(D):
    A, b = cases.system("poisson 33x31")
    S = attach(D, A, "identity")
    full = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER)
    again = S.solve_refined(gpu(b), full.x, rtol_sq=1e-8)
    assert again.status == D._lib.OK and again.iterations == 0 and again.outer_steps == 0 and torch.equal(again.x, full.x)
    zero = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=0)
    assert zero.status == D._lib.MAX_ITER and zero.iterations == 0 and zero.outer_steps == 0 and not zero.x.any() and zero.final_res == 1.0
    ref = cases.restated("poisson 33x31", "identity", 1e-20)
    cap = ref["inner_counts"][0] + 5
    capped = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cap)                 # the cap is reached inside the second inner solve
    assert capped.status == D._lib.MAX_ITER and capped.iterations == cap and capped.outer_steps == 2
    assert len(capped.res_history) == cap + 1 and capped.final_res == capped.outer_history[-1]
    one = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER, max_outer=1)
    assert one.status == D._lib.MAX_ITER and one.outer_steps == 1 and one.final_res > 1e-16       # fp32 alone does not get there


def test_new_values_are_used(D):
    A, b = cases.system("poisson 40x40")
    S = attach(D, A, "jacobi")
    x1 = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER).x.cpu().numpy()
    S.update_values(2.0 * A.data)
    S.set_preconditioner(D.Jacobi())
    res = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER)
    check_solution(D, 2.0 * A, b, res, 1e-20)
    x2 = res.x.cpu().numpy()
    assert np.linalg.norm(x2 - 0.5 * x1) <= 1e-9 * np.linalg.norm(x1)
    # M = I, nothing between update_values and the solve: it is update_values that drops the fp32 copy of the old values
    S = attach(D, A, "identity")
    x1 = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER).x.cpu().numpy()
    S.update_values(2.0 * A.data)
    res = S.solve_refined(gpu(b), rtol_sq=1e-20, max_iter=cases.MAX_ITER)
    check_solution(D, 2.0 * A, b, res, 1e-20)
    assert np.linalg.norm(res.x.cpu().numpy() - 0.5 * x1) <= 1e-9 * np.linalg.norm(x1)


def same_bits(a, b):
    return (a.iterations == b.iterations and a.status == b.status and np.array_equal(a.res_history, b.res_history, equal_nan=True)
            and np.array_equal(a.x.cpu().numpy(), b.x.cpu().numpy(), equal_nan=True))


def refused(D, S, bt, match, call, **solve_kw):
    """a plain solve in the refused state, the refusal, and the same plain solve again on the same handle: bit for bit what it was"""
    L = D._lib
    before = S.solve(bt, **solve_kw)
    with pytest.raises(L.DpcgError, match=match) as e:
        call()
    assert e.value.status == L.ERR_INVALID
    assert same_bits(S.solve(bt, **solve_kw), before)


def test_refusals_leave_the_handle_as_it_was(D):
    A, b = cases.system("shifted 32x32")
    bt = gpu(b)
    L = D._lib
    S = attach(D, A, "jacobi")
    refused(D, S, bt, "inner_rtol_sq", lambda: S.solve_refined(bt, inner_rtol_sq=0.0))
    refused(D, S, bt, "max_outer", lambda: S.solve_refined(bt, max_outer=0))
    refused(D, S, bt, "max_iter", lambda: S.solve_refined(bt, max_iter=-1))
    x = torch.empty_like(bt)
    for flags in (L.SINGLE_REDUCTION, L.NO_GRAPH | L.NO_SMALL):
        refused(D, S, bt, "flags", lambda: L.check(L.lib().dpcg_solve_refined(
            S._h, bt.data_ptr(), None, x.data_ptr(), 1e-8, 0.0, 100, 1e-6, 16, flags, None, None, None, None, None, None, None)))
    assert L.check(L.lib().dpcg_solve_refined(S._h, bt.data_ptr(), None, x.data_ptr(), 1e-8, 0.0, 1000, 1e-6, 16, L.NO_GRAPH, None, None, None,
                                              None, None, None, None)) == L.OK
    S.solve_refined(bt)                                      # (the fp32 copies exist when the next refusals come)
    S.set_preconditioner(D.IC0())
    refused(D, S, bt, "Jacobi", lambda: S.solve_refined(bt))                     # IC(0) attached, before and after
    S2 = attach(D, A, "jacobi")
    S2.set_deflation(np.ones((A.shape[0], 1)))
    refused(D, S2, bt, "deflation", lambda: S2.solve_refined(bt))
    N = R.shifted_laplacian((32, 32), 3, shift=0.0)
    S3 = attach(D, N, "identity")
    S3.set_nullspace("constant", check_tol=0.0)
    refused(D, S3, bt, "null space", lambda: S3.solve_refined(bt))


def test_overflow_is_refused_by_name(D):
    """the one refusal that comes after the driver has begun to allocate and convert: the handle is still what it was"""
    A, b = cases.system("poisson 5x7")
    bt = gpu(b)
    B = A.copy()
    B.data[7] = 1e39
    S = attach(D, B, "identity")
    refused(D, S, bt, "matrix value 7 ", lambda: S.solve_refined(bt), max_iter=50)
    B = A.copy()
    k = int(B.indptr[3] + np.flatnonzero(B.indices[B.indptr[3]:B.indptr[4]] == 3)[0])
    B.data[k] = 1e-39
    S = attach(D, B, "jacobi")
    refused(D, S, bt, "reciprocal diagonal entry 3 ", lambda: S.solve_refined(bt), max_iter=50)


@pytest.mark.parametrize("pre", ["identity", "jacobi"])
def test_plain_solve_keeps_its_bits(D, pre):
    """solve() on a handle that has run solve_refined against a fresh handle's solve(), histories included"""
    for name in ("poisson 33x31", "poisson 271x259"):
        A, b = cases.system(name)
        bt = gpu(b)
        fresh = attach(D, A, pre).solve(bt, max_iter=4000)
        S = attach(D, A, pre)
        S.solve_refined(bt, max_iter=4000)
        after = S.solve(bt, max_iter=4000)
        assert fresh.status == D._lib.OK
        assert after.iterations == fresh.iterations and after.status == fresh.status and after.final_res == fresh.final_res
        assert torch.equal(after.x, fresh.x) and np.array_equal(after.res_history, fresh.res_history)
        assert math.isfinite(after.seconds)
