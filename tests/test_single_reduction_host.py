"""The single-reduction recurrence (DPCG_SINGLE_REDUCTION) on the host: what tests/single_reduction_restatement.py computes, and that
the flag and its getter are declared, exported and bound.  No GPU."""
import pathlib
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O, c_oracle as CO
import single_reduction_restatement as R

ROOT = pathlib.Path(__file__).resolve().parents[1]
RTOL_SQ = 1e-8

SYSTEMS = {"poisson2d_32": lambda: O.poisson2d(32), "poisson3d_12": lambda: O.poisson3d(12)}
# updates to <r,r>/<b,b> < 1e-8 with Jacobi, b = O.rhs(n, 0): the oracle's standard recurrence / the single-reduction one, as measured
# on these systems -- the same count, so the difference allowed is 0
COUNTS = {"poisson2d_32": (64, 64), "poisson3d_12": (30, 30)}


def _true_res(A, b, x):
    r = b - A @ x
    return float(r @ r) / float(b @ b)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_converges_to_the_reference_criterion_on_the_true_residual(name):
    # <b - A x, b - A x> / <b,b> of the returned x, on these systems:
    #   poisson2d_32: oracle's standard solve 9.629414436328927e-09, single reduction 9.629414436323777e-09
    #   poisson3d_12: oracle's standard solve 4.7225666751544536e-09, single reduction 4.72256667515167e-09
    # The standard solve's TRUE residual meets rtol_sq = 1e-8 itself (it leaves no excess over it), so the margin is none: the single-
    # reduction x has to meet rtol_sq on the true residual too.
    A = SYSTEMS[name]()
    n = A.shape[0]
    b, dinv = O.rhs(n, 0), O.jacobi_dinv(A)
    _, it, hist, x = CO.pcg(A, b, "jacobi", dinv=dinv, rtol=RTOL_SQ)
    s = R.solve(A, b, dinv=dinv, rtol_sq=RTOL_SQ)
    print(name, "standard", it, _true_res(A, b, x), "single reduction", s.iterations, _true_res(A, b, s.x))
    assert _true_res(A, b, x) < RTOL_SQ                      # what the margin is taken from
    assert s.status == R.OK and s.res_history.size == s.iterations + 1 and s.res_history[-1] < RTOL_SQ
    assert _true_res(A, b, s.x) < RTOL_SQ
    assert (it, s.iterations) == COUNTS[name]
    assert abs(s.iterations - it) <= abs(COUNTS[name][0] - COUNTS[name][1])
    # the first test is the reference's, on z0 (cg.py:66); with init_check_r on r0
    z0 = dinv * b
    assert s.res_history[0] == np.dot(z0, z0) / np.dot(b, b)
    # (the oracle adds the same positive terms in another order: each sum within n eps of the exact one, the ratio of two within 4 n eps)
    assert abs(s.res_history[0] - hist[0]) <= 4 * n * np.finfo(float).eps * hist[0]
    assert R.solve(A, b, dinv=dinv, init_check_r=True, max_iter=0).res_history[0] == 1.0


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_without_a_preconditioner_gamma_is_rho_bit_for_bit(name):
    A = SYSTEMS[name]()
    b = O.rhs(A.shape[0], 1)
    s = R.solve(A, b, init_check_r=True)
    assert s.status == R.OK and s.iterations > 5 and np.array_equal(s.gamma, s.rho)
    s = R.solve(A, b)                                        # (the first test on z0 = r0: the same sum again)
    assert np.array_equal(s.gamma, s.rho)


def test_caps_of_zero_and_one_update():
    A = O.poisson2d(32)
    n = A.shape[0]
    b, x0, dinv = O.rhs(n, 0), O.rhs(n, 5), O.jacobi_dinv(A)
    for start in (None, x0):
        s0 = R.solve(A, b, dinv=dinv, x0=start, max_iter=0)
        assert s0.iterations == 0 and s0.status == R.MAX_ITER and s0.res_history.size == 1
        assert np.array_equal(s0.x, np.zeros(n) if start is None else start)           # x is not touched
        s1 = R.solve(A, b, dinv=dinv, x0=start, max_iter=1)
        assert s1.iterations == 1 and s1.status == R.MAX_ITER and s1.res_history.size == 2
        # one update IS the steepest-descent step of the standard recurrence: alpha_0 = <r,z> / <z,Az>, p_0 = z_0
        r0 = b if start is None else b - CO.spmv(A, start)
        z0 = dinv * r0
        alpha = np.dot(r0, z0) / np.dot(z0, CO.spmv(A, z0))
        assert np.array_equal(s1.x, (np.zeros(n) if start is None else start) + alpha * z0)
        r1 = r0 - alpha * CO.spmv(A, z0)
        assert s1.res_history[1] == np.dot(r1, r1) / np.dot(b, b)
    full = R.solve(A, b, dinv=dinv)
    capped = R.solve(A, b, dinv=dinv, max_iter=10)
    assert capped.iterations == 10 and np.array_equal(capped.res_history, full.res_history[:11])
    assert R.solve(A, b, dinv=dinv, atol_sq=1e300).iterations == 0                      # atol_sq: <r,r> itself below it
    assert R.solve(A, np.zeros(n), dinv=dinv).status == R.BREAKDOWN                     # <b,b> = 0 -> 0/0, as on every device path


def test_a_system_that_is_not_positive_definite_gives_the_documented_status():
    # den = <z,Az> = 0 at the first update: alpha = inf, the residual inf (not yet NaN: the solve goes on, as k_pcg_chip does on its
    # <p,Ap>), NaN one update later -> DPCG_BREAKDOWN with the count of the update that saw it
    A = sp.diags([1.0, -1.0]).tocsr()
    s = R.solve(A, np.array([1.0, 1.0]))
    assert s.status == R.BREAKDOWN and s.iterations == 2 and np.isinf(s.res_history[1]) and np.isnan(s.res_history[2])
    # an indefinite system on which den stays away from zero runs like any other: no status of its own
    B = sp.diags([1.0, 2.0, -3.0]).tocsr()
    t = R.solve(B, np.array([1.0, 2.0, 1.0]), max_iter=10)
    assert t.status in (R.OK, R.MAX_ITER) and np.all(np.isfinite(t.res_history))


def test_the_chip_tree_of_the_restatement_is_the_oracles():
    """One standard dot product of a known solve: the oracle's first test <z0,z0> / <b,b> with its form "chip"."""
    A = O.poisson3d(41)
    n = A.shape[0]
    b, dinv = O.rhs(n, 0), O.jacobi_dinv(A)
    per = (n + 255) // 256
    tree = {"spmv_grid": 1, "nrb": 1, "cyclic": 0, "vec_grid": 1, "form": "chip", "rows_per_workgroup": per}
    _, it, hist, _ = CO.pcg(A, b, "jacobi", dinv=dinv, max_iter=0, device_tree=tree)
    z0 = dinv * b
    assert it == 0 and hist[0] == R.chip_dot(z0, z0, per) / R.chip_dot(b, b, per)
    assert hist[0] != np.dot(z0, z0) / np.dot(b, b)         # (another order, other bits: the comparison above can fail)
    # the wave tree, lane by lane: quads, then the four quads of a row, then the four rows, the higher half first
    v = np.random.default_rng(0).standard_normal(64)
    rows = []
    for r in range(4):
        q = [(v[16 * r + 4 * k] + v[16 * r + 4 * k + 1]) + (v[16 * r + 4 * k + 2] + v[16 * r + 4 * k + 3]) for k in range(4)]
        rows.append((q[3] + q[2]) + (q[1] + q[0]))
    assert R.wave_tree(v) == (rows[3] + rows[2]) + (rows[1] + rows[0])


def test_flag_and_getter_are_declared_exported_and_bound():
    from deeppreconditioning_amd import _lib
    header = (ROOT / "include" / "dpcg.h").read_text()
    assert re.search(r"DPCG_SINGLE_REDUCTION\s*=\s*256\b", header) and _lib.SINGLE_REDUCTION == 256
    assert re.search(r"^int\s+dpcg_get_last_recurrence\(dpcg_handle_t h, int \*recurrence\);", header, flags=re.M)
    assert _lib.SIGNATURES["dpcg_get_last_recurrence"][1][0] is _lib._p and _lib.RECURRENCES == ("standard", "single_reduction")
    flags = [_lib.INIT_CHECK_R, _lib.SPMV_F32, _lib.NO_GRAPH, _lib.NO_SMALL, _lib.VAL32_IF_LOSSLESS, _lib.NO_FUSE, _lib.NO_TEAM, _lib.TEAM,
             _lib.SINGLE_REDUCTION]
    assert len(set(flags)) == 9 and all(f & (f - 1) == 0 for f in flags)            # one bit each, none shared
    so = _lib.build()
    exported = set(re.findall(r" T (dpcg_[a-z0-9_]+)", subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout))
    assert "dpcg_get_last_recurrence" in exported


def test_python_interface_keeps_its_defaults():
    import dataclasses
    import inspect
    from deeppreconditioning_amd import cg, operators
    f = {x.name: x for x in dataclasses.fields(operators.SolveResult)}
    assert f["recurrence"].default == "standard" and list(f)[-1] == "recurrence"        # existing construction sites keep working
    for fn in (operators.CsrSystem.solve, cg.preconditioned_conjugate_gradient, cg.conjugate_gradient):
        prm = inspect.signature(fn).parameters["recurrence"]
        assert prm.default == "standard" and prm.kind is inspect.Parameter.KEYWORD_ONLY, fn
