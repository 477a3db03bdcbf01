"""The single-reduction recurrence in the whole-chip kernel (DPCG_SINGLE_REDUCTION, dpcg_chip_sr.hip) against its numpy restatement
(tests/single_reduction_restatement.py) with the handle's chip tree: history, count, status and x EQUAL, on the smallest systems that
reach each instantiation.  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C
import os
import pathlib
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from oracle import oracle as O
import single_reduction_restatement as R
from gpu_streams import concurrent_side_stream

pytestmark = pytest.mark.gpu

SR = "single_reduction"


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()  # raises if the HIP extension is missing: no silent fallback
    return pkg


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tree(S):
    ci = S.chip_info()
    assert ci["chip_by_default"] and ci["workgroups"] == 256 and ci["threads"] == 512, ci
    return {"rows_per_workgroup": ci["rows_per_workgroup"]}


def _same(res, ref, x_ref=None):
    assert res.recurrence == SR
    assert res.iterations == ref.iterations and res.status == ref.status, (res.iterations, ref.iterations, res.status, ref.status)
    assert np.array_equal(res.res_history, ref.res_history), int(np.argmax(res.res_history != ref.res_history))
    assert np.array_equal(res.x.cpu().numpy(), ref.x if x_ref is None else x_ref)


@pytest.fixture(scope="module")
def p41(D):
    """3-D 41^3 with Jacobi: the system most cases share, its handle and its restated solve (computed once, never modified)."""
    A = O.poisson3d(41)
    n = A.shape[0]
    b, dinv = O.rhs(n, 0), O.jacobi_dinv(A)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    ref = R.solve(A, b, dinv=dinv, tree=_tree(S))
    yield A, b, dinv, S, ref
    S.close()


@pytest.mark.parametrize("name,make,kind,max_iter,rpt", [
    ("poisson3d_41", lambda: O.poisson3d(41), "none", 1024, 2),           # 68 921 rows, 2 rows a thread, M = I (Jacobi: the shared fixture below)
    ("poisson2d_300", lambda: O.poisson2d(300), "jacobi", 1024, 2),       # 90 000 rows, rows of 5 entries
    ("poisson3d_65", lambda: O.poisson3d(65), "jacobi", 30, 4),           # 274 625 rows: 4 rows a thread
    ("poisson2d_730", lambda: O.poisson2d(730), "jacobi", 30, 8)])        # 532 900 rows of 5 entries: 8 rows a thread, x in memory
def test_equals_the_restatement_bit_for_bit(D, name, make, kind, max_iter, rpt):
    A = make()
    n = A.shape[0]
    b = O.rhs(n, 0)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi() if kind == "jacobi" else None)
    tree = _tree(S)
    rows_a_thread = (tree["rows_per_workgroup"] + 511) // 512
    assert rows_a_thread <= rpt and (rpt == 2 or rows_a_thread > rpt // 2)           # the instantiation the case is here for
    res = S.solve(_dev(b), max_iter=max_iter, recurrence=SR)
    ref = R.solve(A, b, dinv=O.jacobi_dinv(A) if kind == "jacobi" else None, max_iter=max_iter, tree=tree)
    _same(res, ref)
    assert ref.status == (R.OK if max_iter == 1024 else R.MAX_ITER)
    if kind == "none":
        assert np.array_equal(ref.gamma, ref.rho)
    S.close()


def test_jacobi_to_convergence_determinism_and_separation(D, p41):
    """41^3 with Jacobi to convergence; two runs give identical bits; a standard solve of the same handle before and after is bit-identical
    to one on a fresh handle (the variant shares the granule table and the slots with it and leaves nothing behind)."""
    A, b, dinv, S, ref = p41
    before = S.solve(_dev(b))
    one = S.solve(_dev(b), recurrence=SR)
    two = S.solve(_dev(b), recurrence=SR)
    after = S.solve(_dev(b))
    _same(one, ref)
    assert ref.status == R.OK
    assert np.array_equal(one.res_history, two.res_history) and torch.equal(one.x, two.x) and two.recurrence == SR
    fresh = D.CsrSystem.from_any(A, reorder=None)
    fresh.set_preconditioner(D.Jacobi())
    std = fresh.solve(_dev(b))
    fresh.close()
    for r in (before, after):
        assert r.recurrence == "standard" and np.array_equal(r.res_history, std.res_history) and torch.equal(r.x, std.x)
    assert not np.array_equal(std.res_history, one.res_history)          # (another recurrence, other bits: it WAS the variant)
    # the same switch on the drop-in functions
    from deeppreconditioning_amd.cg import preconditioned_conjugate_gradient
    d = preconditioned_conjugate_gradient(S, _dev(b), D.Jacobi(), recurrence=SR, details=True)
    assert d.recurrence == SR and np.array_equal(d.res_history, ref.res_history)


def test_x0_init_check_and_caps(D, p41):
    A, b, dinv, S, ref = p41
    n = A.shape[0]
    tree = _tree(S)
    x0 = O.rhs(n, 7)
    x_in = _dev(x0)
    keep = x_in.clone()
    _same(S.solve(_dev(b), x_in, recurrence=SR), R.solve(A, b, dinv=dinv, x0=x0, tree=tree))
    assert torch.equal(x_in, keep)                                       # x0 is not modified
    _same(S.solve(_dev(b), flags=D._lib.INIT_CHECK_R, recurrence=SR), R.solve(A, b, dinv=dinv, init_check_r=True, tree=tree))
    for max_iter in (0, 1):
        for start in (None, x0):
            r = S.solve(_dev(b), None if start is None else _dev(start), max_iter=max_iter, recurrence=SR)
            e = R.solve(A, b, dinv=dinv, x0=start, max_iter=max_iter, tree=tree)
            _same(r, e)
            assert r.iterations == max_iter and r.status == 1
    rz = S.solve(_dev(np.zeros(n)), recurrence=SR)                       # <b,b> = 0 -> 0/0: breakdown, as on every other path
    assert rz.status == 2 and rz.iterations == 0 and rz.recurrence == SR


def test_a_handle_the_library_reordered(D):
    A = O.unstructured_like(O.poisson3d(41), seed=1)                     # scattered numbering + D A D scaling: RCM inside the library
    n = A.shape[0]
    b = O.rhs(n, 0)
    S = D.CsrSystem.from_any(A)
    S.set_preconditioner(D.Jacobi())
    assert S.reordered
    perm = S.permutation()
    B = A[perm][:, perm].tocsr()
    B.sort_indices()
    res = S.solve(_dev(b), recurrence=SR)
    ref = R.solve(B, b[perm], dinv=O.jacobi_dinv(B), tree=_tree(S))
    xs = res.x.cpu().numpy()
    _same(res, ref, x_ref=ref.x[np.argsort(perm)])                       # b and x in the caller's numbering
    assert ref.status == R.OK and np.array_equal(xs[perm], ref.x)
    S.close()


def test_with_every_granule_written_through(D):
    """DPCG_CHIP_LOCAL=0 (read once per process, so a child process): no plainly stored copies -- the form any placement of the
    workgroups falls back to.  Same bits as the restatement."""
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, "tests")
        import numpy as np, torch
        import deeppreconditioning_amd as D
        from oracle import oracle as O
        import single_reduction_restatement as R
        A = O.poisson3d(41)
        n = A.shape[0]
        b = O.rhs(n, 3)
        S = D.CsrSystem.from_any(A, reorder=None)
        S.set_preconditioner(D.Jacobi())
        res = S.solve(torch.from_numpy(b).cuda(), recurrence="single_reduction")
        ref = R.solve(A, b, dinv=O.jacobi_dinv(A), tree={"rows_per_workgroup": S.chip_info()["rows_per_workgroup"]})
        assert res.recurrence == "single_reduction" and res.iterations == ref.iterations and res.status == ref.status == 0
        assert np.array_equal(res.res_history, ref.res_history) and np.array_equal(res.x.cpu().numpy(), ref.x)
        print("ok", ref.iterations)
    """)
    env = dict(os.environ, DPCG_CHIP_LOCAL="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=str(pathlib.Path(__file__).resolve().parents[1]))
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_refusals_name_their_reason_and_leave_the_handle_as_it_was(D, p41):
    A, b, dinv, S, ref = p41
    n = A.shape[0]
    std = S.solve(_dev(b), max_iter=20)

    def refused(system, rhs, fragment, **kw):
        with pytest.raises(D._lib.DpcgError) as e:
            system.solve(rhs, recurrence=SR, **kw)
        assert e.value.status == D._lib.ERR_INVALID and fragment in str(e.value), str(e.value)

    refused(S, _dev(b), "fp64 only", flags=D._lib.SPMV_F32)
    refused(S, _dev(b), "x_true", x_true=_dev(O.rhs(n, 4)))
    refused(S, _dev(b), "whole-chip kernel only", flags=D._lib.NO_SMALL)
    again = S.solve(_dev(b), max_iter=20)                               # the previous state is intact
    assert again.recurrence == "standard" and np.array_equal(again.res_history, std.res_history) and torch.equal(again.x, std.x)
    S.set_preconditioner(D.IC0("solve"))
    refused(S, _dev(b), "M = I or Jacobi")
    assert S.solve(_dev(b), max_iter=5).iterations == 5                  # ... and IC(0) still solves
    S.set_preconditioner(D.Jacobi())
    _same(S.solve(_dev(b), recurrence=SR), ref)
    small = D.CsrSystem.from_any(O.poisson2d(32), reorder=None)         # 1 024 rows
    small.set_preconditioner(D.Jacobi())
    refused(small, _dev(O.rhs(1024, 0)), "whole-chip kernel's size")
    assert small.solve(_dev(O.rhs(1024, 0))).status == 0
    small.close()
    with pytest.raises(ValueError):
        S.solve(_dev(b), recurrence="pipelined")


def test_eight_rows_a_thread_of_seven_entries_are_refused(D):
    """81^3 = 531 441 rows of 7 entries: eight rows a thread spill even with x in memory, so the variant stops at
    524 288 rows for rows of more than 5 entries -- and says so."""
    A = O.poisson3d(81)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    assert S.chip_info()["chip_by_default"] and (S.chip_info()["rows_per_workgroup"] + 511) // 512 == 5
    b = _dev(O.rhs(A.shape[0], 0))
    with pytest.raises(D._lib.DpcgError) as e:
        S.solve(b, max_iter=30, recurrence=SR)
    assert e.value.status == D._lib.ERR_INVALID and "at most 5 entries beyond 524 288 rows" in str(e.value)
    assert S.solve(b, max_iter=30).iterations == 30
    S.close()


def test_falls_back_to_the_standard_recurrence_when_somebody_else_holds_cus(D, p41):
    """As test_one_launch_solves_when_somebody_else_holds_cus: 96 workgroups that take a whole CU each (dpcg_debug_occupy) keep the kernel
    from becoming co-resident; the SAME call then solves through the launches with the standard recurrence and says so."""
    import time
    A, b, dinv, S, ref = p41
    multi = S.solve(_dev(b), flags=D._lib.NO_SMALL)
    side = concurrent_side_stream(D)         # (a plain new stream may share the solve's hardware queue: tests/gpu_streams.py)
    torch.cuda.synchronize()
    D._lib.check(D._lib.lib().dpcg_debug_occupy(96, 400.0, side.cuda_stream))
    time.sleep(0.03)                                                     # the squatters are resident
    t0 = time.perf_counter()
    res = S.solve(_dev(b), recurrence=SR)
    dt_plain = time.perf_counter() - t0
    side.synchronize()
    assert res.recurrence == "standard" and res.status == 0
    assert np.array_equal(res.res_history, multi.res_history) and torch.equal(res.x, multi.x)      # it WAS the multi-launch path
    _same(S.solve(_dev(b), recurrence=SR), ref)                          # the CUs are free again: the variant again
    # DPCG_TEAM ("that kernel whatever the other flags say") beside the flag: the fall-back still goes to the launches, not through the
    # standard whole-chip kernel and a second 20 ms wait
    D._lib.check(D._lib.lib().dpcg_debug_occupy(96, 400.0, side.cuda_stream))
    time.sleep(0.03)
    t0 = time.perf_counter()
    res = S.solve(_dev(b), flags=D._lib.TEAM, recurrence=SR)
    dt = time.perf_counter() - t0
    side.synchronize()
    assert res.recurrence == "standard" and np.array_equal(res.res_history, multi.res_history)
    assert dt < dt_plain + 0.012, (dt, dt_plain)                         # one bounded wait (20 ms) like the call above, not a second one on top
    _same(S.solve(_dev(b), flags=D._lib.TEAM, recurrence=SR), ref)


def test_batch_treats_the_flag_per_system(D, p41):
    from deeppreconditioning_amd.batch import solve_batch
    A, b, dinv, S, ref = p41
    S2 = D.CsrSystem.from_any(A, reorder=None)
    S2.set_preconditioner(D.Jacobi())
    b2 = O.rhs(A.shape[0], 5)
    out = solve_batch([S, S2], [_dev(b), _dev(b2)], flags=D._lib.SINGLE_REDUCTION)
    ref2 = R.solve(A, b2, dinv=dinv, tree=_tree(S2))
    for r, e, h in zip(out, (ref, ref2), (S, S2)):
        ran = C.c_int(-1)
        D._lib.check(D._lib.lib().dpcg_get_last_recurrence(h._h, C.byref(ran)))
        assert ran.value == 1 and r.iterations == e.iterations and r.status == 0 and np.array_equal(r.x.cpu().numpy(), e.x)
        assert r.recurrence == SR                                         # SolveResult names the recurrence that RAN, through the batch too
    # a plain batch of the same handles afterwards: the standard recurrence, and the report says so (C getter and SolveResult)
    plain = solve_batch([S, S2], [_dev(b), _dev(b2)])
    std = S.solve(_dev(b))
    for r, h in zip(plain, (S, S2)):
        ran = C.c_int(-1)
        D._lib.check(D._lib.lib().dpcg_get_last_recurrence(h._h, C.byref(ran)))
        assert ran.value == 0 and r.recurrence == "standard" and r.status == 0
    assert plain[0].iterations == std.iterations and torch.equal(plain[0].x, std.x)
    S.solve(_dev(b), recurrence=SR)
    plain = solve_batch([S, S2], [_dev(b), _dev(b2)], flags=D._lib.NO_SMALL)        # ... and through the streams of the multi-launch path
    assert [r.recurrence for r in plain] == ["standard", "standard"]
    small = D.CsrSystem.from_any(O.poisson2d(32), reorder=None)
    small.set_preconditioner(D.Jacobi())
    with pytest.raises(D._lib.DpcgError) as e:
        solve_batch([S, small], [_dev(b), _dev(O.rhs(1024, 0))], flags=D._lib.SINGLE_REDUCTION)
    assert e.value.status == D._lib.ERR_INVALID and "whole-chip kernel's size" in str(e.value)
    small.close()
    S2.close()
