"""dpcg_solve_bicgstab at its edges (bicgstab_edge_cases.py has the systems; test_bicgstab_edges_host.py asserts the conditions on them).

  A  later trips of the software-pipelined vector passes and more than 256 partials: a child process whose grid DPCG_VEC_GRID holds to
     1 and 3 workgroups, and 257 x 257 / 725 x 725 in process at their natural grids (259 and 1024 workgroups; the SpMV's 2048 with the
     CSR-stream kernel forced)
  B  A's tile, vector and mixed-tile SpMV with a second vector in the dot epilogue (<rhat, A ph>, <s, A sh>), forced and by default
  C  one handle through every preconditioner, through update_values and through a PCG solve in between: the bits of a fresh handle
  D  every breakdown site on inputs whose arithmetic is exact: the restatement's status, count, history and x, bit for bit; non-finite
     and zero b; the half-step exit with five workgroups

Every numeric comparison is test_bicgstab_gpu.py's short-run rule against bicgstab_restatement.bicgstab: K updates, history[0..K] and x
within SHORT_TOL = 1e-10.  No count is asserted at a size where the two CPU summation orders were not shown to agree on it.
"""

import json
import os
import pathlib
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bicgstab_cases as C
import bicgstab_edge_cases as E
import bicgstab_restatement as R
import test_bicgstab_gpu as T

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
gpu, check_short, healthy = T.gpu, T.check_short, T.healthy


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def precond(D, A, name, pre):
    if pre == "none":
        return None
    if pre == "jacobi":
        return D.Jacobi()
    if pre == "csr":
        return D.CsrPreconditioner(C.neumann_series_csr(A))
    mode, kw = C.ilut_mode(pre)
    return D.ILUT(mode, **kw)


def attach(D, name, pre):
    A = E.matrix(name)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(precond(D, A, name, pre))
    return S


def short_run(D, name, pre, S=None):
    """the K_OF[pair] updates of a pair on a fresh handle (or S), held to the restatement"""
    k = E.K_OF.get((name, pre), E.K)
    S = S or attach(D, name, pre)
    res = S.solve_bicgstab(gpu(E.rhs(name)), rtol_sq=E.RTOL_SQ, max_iter=k)
    check_short(res, E.restated(name, pre, k), f"{name} {pre}")
    return res


def same_bits(res, ref, what):
    assert res.iterations == ref.iterations and res.status == ref.status, (what, res.iterations, res.status, ref.iterations, ref.status)
    assert np.array_equal(res.res_history, ref.res_history, equal_nan=True) and torch.equal(res.x, ref.x), what


# ---- A. trips and partial counts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", E.CHILD)
def test_later_trips_of_the_vector_passes(D, grid):
    name, pairs, lanes, trips = E.CHILD[grid]
    env = {**os.environ, "PYTHONPATH": os.pathsep.join([str(ROOT)] + [p for p in [os.environ.get("PYTHONPATH")] if p]),
           "DPCG_VEC_GRID": str(grid)}
    proc = subprocess.run([sys.executable, str(ROOT / "tests" / "bicgstab_edges_child.py")], capture_output=True, text=True, cwd=ROOT,
                          env=env, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    out = json.loads([line for line in proc.stdout.splitlines() if line.startswith("{")][-1])
    assert out["name"] == name and out["vec_grid"] == grid, (out["name"], out["vec_grid"])
    assert sorted(out["runs"]) == sorted(C.PRECONDS + [E.CHILD_X0_PRE + "_x0"])
    for tag, rec in out["runs"].items():
        pre, x0 = (tag[:-3], True) if tag.endswith("_x0") else (tag, False)
        res = types.SimpleNamespace(iterations=rec["iterations"], status=rec["status"], res_history=np.array(rec["history"]),
                                    x=torch.tensor(rec["x"], dtype=torch.float64), final_res=rec["final_res"], recurrence="bicgstab")
        check_short(res, E.restated(name, pre, E.K, False, x0), f"{name} {tag} on {grid} workgroup(s), {trips} trips")
        assert res.iterations == E.K


@pytest.mark.parametrize("name,pre", E.NATURAL)
def test_natural_grids_beyond_256_partials(D, name, pre):
    S = attach(D, name, pre)
    geo = S.reduction_geometry()
    assert geo["vec_grid"] == E.VEC_GRID[name], geo
    if name == "725x725_pe3":                              # the tile plan by default; its LDS tiles leave six workgroups a CU: 1536
        print(f"{name}: {geo['spmv_kernel']} kernel on {geo['spmv_grid']} workgroups")
        assert S.info()["spmv_kernel"] == "tile" and 1024 < geo["spmv_grid"] <= 2048, (S.info()["spmv_kernel"], geo["spmv_grid"])
    short_run(D, name, pre, S)
    S.close()


@pytest.mark.parametrize("pre", ["none", "jacobi"])
def test_all_eight_slots_of_the_spmv_partials(D, monkeypatch, pre):
    """2054 row blocks through the CSR-stream kernel: its grid is the full 2048, so passes S and X read all eight slots of
    EarlyPartials (the tile plan this system takes by default stops at six workgroups a CU)"""
    monkeypatch.setenv("DPCG_SPMV_KERNEL", "stream")
    name = "725x725_pe3"
    S = attach(D, name, pre)
    geo = S.reduction_geometry()
    assert S.info()["spmv_kernel"] == "stream" and geo["spmv_grid"] == 2048 and geo["vec_grid"] == 1024, (S.info()["spmv_kernel"], geo)
    short_run(D, name, pre, S)
    S.close()


# ---- B. every SpMV plan under BiCGStab ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", C.PRECONDS)
@pytest.mark.parametrize("kernel,name", E.FORCED)
def test_forced_spmv_plans(D, monkeypatch, kernel, name, pre):
    monkeypatch.setenv("DPCG_SPMV_KERNEL", kernel)
    S = attach(D, name, pre)
    assert S.info()["spmv_kernel"] == kernel, S.info()
    short_run(D, name, pre, S)
    S.close()


@pytest.mark.parametrize("pre", C.PRECONDS)
@pytest.mark.parametrize("name", E.VECTOR_BY_DEFAULT)
def test_the_vector_kernel_by_default(D, name, pre):
    S = attach(D, name, pre)
    geo = S.reduction_geometry()
    print(f"{name}: {geo['spmv_kernel']} kernel, {geo['spmv_tpr']} lanes a row, {geo['spmv_grid']} workgroups")
    assert S.info()["spmv_kernel"] == "vector" and geo["spmv_tpr"] == E.VECTOR_BY_DEFAULT[name], geo
    res = short_run(D, name, pre, S)
    if (name, pre) in E.STOPS_INSIDE:
        assert res.status == D._lib.OK and res.iterations == E.STOPS_INSIDE[(name, pre)]
    S.close()


@pytest.mark.parametrize("pre", C.PRECONDS)
def test_a_tile_plan_with_blocks_that_gather(D, monkeypatch, pre):
    monkeypatch.setenv("DPCG_TILE_MIX_MAX", "30")
    S = attach(D, E.MIX, pre)
    info = S.info()
    assert info["spmv_kernel"] == "tile" and info["spmv_mixed_tiles"] and not info["reordered"], info
    short_run(D, E.MIX, pre, S)
    S.close()


# ---- C. the handle's life ---------------------------------------------------------------------------------------------------------
def test_one_handle_through_every_preconditioner(D):
    name = E.LIFE_SYSTEM
    A, b = E.matrix(name), gpu(E.rhs(name))
    fresh = {}
    for pre in sorted(set(E.LIFE_ORDER)):
        F = attach(D, name, pre)
        fresh[pre] = F.solve_bicgstab(b, rtol_sq=E.RTOL_SQ, max_iter=E.K)
        check_short(fresh[pre], R.bicgstab(A, E.rhs(name), T.device_m(F, name, pre), rtol_sq=E.RTOL_SQ, max_iter=E.K), f"{name} {pre}")
        F.close()
    S = D.CsrSystem.from_any(A, reorder=None)                # the first call has no M: `sh` is made by a later one
    for step, pre in enumerate(E.LIFE_ORDER):
        S.set_preconditioner(precond(D, A, name, pre))
        same_bits(S.solve_bicgstab(b, rtol_sq=E.RTOL_SQ, max_iter=E.K), fresh[pre], f"call {step}: {pre}")
    S.close()


@pytest.mark.parametrize("pre", ["jacobi", "csr"])
def test_update_values_between_two_calls(D, pre):
    old, new = E.LIFE_SYSTEM, E.NEW_VALUES
    Anew, b = E.matrix(new), gpu(E.rhs(new))
    S = attach(D, old, pre)
    short_run(D, old, pre, S)
    S.update_values(Anew.data)
    S.set_preconditioner(precond(D, Anew, new, pre))         # M of the new values
    res = S.solve_bicgstab(b, rtol_sq=E.RTOL_SQ, max_iter=E.K)
    same_bits(res, short_run(D, new, pre), f"{old} -> {new} {pre}")
    S.close()


def test_a_pcg_solve_between_two_calls(D):
    name = E.LIFE_SYSTEM
    b = gpu(E.rhs(name))
    S = attach(D, name, "jacobi")
    one = short_run(D, name, "jacobi", S)
    for flags in (0, D._lib.NO_SMALL):                       # the one-workgroup kernel, then the launches (they use the handle's p, q, z)
        S.solve(b, max_iter=5, flags=flags)                  # (CG on non-symmetric values: whatever it returns)
        same_bits(S.solve_bicgstab(b, rtol_sq=E.RTOL_SQ, max_iter=E.K), one, f"after a PCG solve with flags {flags}")
    S.close()


# ---- D. every breakdown site, exactly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, E.KRON])
@pytest.mark.parametrize("name", E.BREAKDOWNS)
def test_breakdown_sites_bit_for_bit(D, name, copies):
    _, _, _, status, updates, history, x = E.BREAKDOWNS[name]
    rowptr, col, val, b = E.breakdown_system(name, copies)
    S = D.CsrSystem(gpu(rowptr), gpu(col), gpu(val), b.size, reorder=None)
    for max_iter in (2, 1024):
        res = S.solve_bicgstab(gpu(b), rtol_sq=E.RTOL_SQ, max_iter=max_iter)
        got = res.x.cpu().numpy()
        print(f"{name} x {copies}, max_iter {max_iter}: status {res.status} after {res.iterations} updates, history {res.res_history}, x {got[:3]}")
        assert res.status == status == D._lib.BREAKDOWN and res.iterations == updates, (res.status, res.iterations)
        assert np.array_equal(res.res_history, np.array(history)) and np.array_equal(got, np.tile(x, copies))
    S.close()
    healthy(D)


@pytest.mark.parametrize("pre", ["none", "jacobi"])
def test_a_nonfinite_b_and_a_zero_b(D, pre):
    name = "23x23_pe2"
    A, b = E.matrix(name), E.rhs(name).copy()
    x0 = E.x0_of(name)
    b[7] = np.inf
    S = attach(D, name, pre)
    for start in (None, x0):
        res = S.solve_bicgstab(gpu(b), None if start is None else gpu(start), rtol_sq=E.RTOL_SQ)
        ref = R.bicgstab(A, b, E.precond_apply(name, pre), x0=start, rtol_sq=E.RTOL_SQ)
        assert ref["status"] == R.BREAKDOWN and ref["iterations"] == 0
        assert res.status == D._lib.BREAKDOWN and res.iterations == 0 and len(res.res_history) == 1 and np.isnan(res.res_history[0])
        assert np.array_equal(res.x.cpu().numpy(), np.zeros_like(b) if start is None else start)
    healthy(D)
    zero = np.zeros(A.shape[0])
    res = S.solve_bicgstab(gpu(zero), rtol_sq=E.RTOL_SQ, atol_sq=0.0)
    assert res.status == D._lib.BREAKDOWN and res.iterations == 0 and len(res.res_history) == 1 and not res.x.any()
    res = S.solve_bicgstab(gpu(zero), rtol_sq=E.RTOL_SQ, atol_sq=1e-30)
    assert res.status == D._lib.OK and res.iterations == 0 and len(res.res_history) == 1 and not res.x.any()
    healthy(D)
    short_run(D, name, pre, S)                               # the handle is as good as new
    S.close()


def test_the_half_step_exit_with_five_workgroups(D):
    Dg, d, bd = E.half_step_system()
    S = D.CsrSystem.from_any(Dg, reorder=None)
    S.set_preconditioner(D.Jacobi())
    assert S.reduction_geometry()["vec_grid"] == 5
    res = S.solve_bicgstab(gpu(bd), rtol_sq=E.RTOL_SQ)
    print(f"half-step exit: status {res.status} after {res.iterations} updates, history {res.res_history}")
    assert res.status == D._lib.OK and res.iterations == 1 and res.res_history[0] == 1.0 and res.res_history[1] <= E.HALF_BOUND
    np.testing.assert_allclose(res.x.cpu().numpy(), bd / d, rtol=1e-15)
    S.close()
    healthy(D)
