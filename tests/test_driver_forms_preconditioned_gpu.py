"""The PCG driver's solve forms (dpcg_solve.hip: Solve::start, the routing of dpcg_solve) under the preconditioners that users attach
-- FSAI(level=1), ICholT(1, 0.1) multiplied and solved, ILUT(1, 0.1) multiplied and solved, SmoothedAggregation (Jacobi fp64,
Gauss-Seidel, the fp32 cycle) -- against the numpy restatement of the plain loop (tests/driver_restatement.py) whose M is taken from
the handle itself: S.factor(), S.lu_factors(), the device's hierarchy fed to the restatements' V-cycles.  The driver is under test,
not the setups (tests/test_{fsai,ilut,amg}*_gpu.py, tests/test_gpu_parity.py have those).

Cases, systems and seeds: tests/driver_forms_cases.py.  Forms covered, every one asserted from the handle's own answers (`form_of`):
  FSAI, ICholT multiplied   one workgroup (33x31: 1 023 rows; 32x32: 1 024), whole-chip L L^T (6 241 rows), the launches
                            (DPCG_NO_SMALL | DPCG_NO_TEAM; every reordered handle below 6 144 rows; x_true; DPCG_SPMV_F32)
  ICholT solved             the launches, 1 023 .. 1 600 rows, plain and reorder="rcm".  The whole-chip triangular-solve form is offered
                            from 1 024 rows and REFUSES the ICholT(1, 0.1) factor: at 32x32 (natural order) for its 110 dependency levels
                            against the form's 18, at 1 600 rows (16 levels) for rows with fill of up to 13 entries, more than the slots
                            beside A's row.  So that form runs under NONE of these preconditioners; the refusal is asserted instead
                            (test_triangular_solve_form_refuses_the_icholt_factor), and the form's own start-vector, cap and history
                            code runs under IC(0) in tests/test_chip_forms_gpu.py
  ILUT, both modes; AMG     the launches (two-kernel updates by default, three kernels with deferred x under DPCG_NO_FUSE; chunks of 8,
                            of 2 with AMG), 1 023 .. 6 241 rows, plain and reorder="rcm"
per form: a start vector, DPCG_INIT_CHECK_R, the absolute tolerance, caps (0, 1, odd, one below a multiple of any chunk of 2 .. 8); per
preconditioner: DPCG_NO_GRAPH / DPCG_NO_FUSE / DPCG_DRIVER_ALTERNATE / want_history=False bit for bit, x_true (plain and reordered),
DPCG_SPMV_F32, DPCG_VAL32_IF_LOSSLESS, guess=, update_values, and with AMG the forms one after the other on one handle.

Comparison (the rule of tests/test_deflation_gpu.py): a COUNT case -- stop margin >= 1.2 and the restatement's own history moving by
less than 1e-11 under a 1e-16 perturbation of b, both evaluated here with the device's M -- has the restatement's status, count and
history (1e-10) and, capped, its x (rtol 1e-9, atol 1e-12); every other case must converge with a true residual below the threshold
and not one update late (a capped one: end at its cap), and agree with the restatement's history (1e-10) over the leading entries that
each move by less than 1e-11 under the perturbation.  driver_forms_cases.COUNT_CASES names the count cases -- as the complement of the
shorter list NOT_COUNT_CASES, so that a new case is a count case unless named -- and one that drifts out of the class fails.  PCG with
ILUT(1, 0.1) never reaches a stopping test other than the cap (M is not symmetric; the restatement's history rises to 10 .. 20 by
update 40): its "atol" case ends on the first test (ILUT solved) or after one update (ILUT multiplied), where its history is lowest.

Largest history difference of the count cases measured on an MI355X (printed by every run): FSAI 1.8e-13, ICholT 4.2e-13,
ILUT 2.6e-15, AMG 9.1e-13; err_history 5.5e-13 (AMG, Gauss-Seidel); guess=: start vector 2.2e-15 of |x0| against a bar of 1.6e-14,
first history entry 1.0e-12.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import driver_forms_cases as C
import driver_restatement as R

pytestmark = pytest.mark.gpu

HIST_RTOL = 1e-10


@pytest.fixture(scope="module")
def D():
    """The package -- and, when the module is done, every handle it built is closed again: a handle owns a capture stream, captured
    graphs and pinned memory, and some thirty of them left open would stay with the process for every test module that runs after this
    one (tests of other modules read the device's free memory, or need the whole chip for a one-launch form)."""
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    yield pkg
    torch.cuda.synchronize()
    for S in _HANDLES.values():
        S.close()
    _HANDLES.clear()
    _APPLY.clear()
    import gc
    gc.collect()
    pkg.operators.release_cached_memory()          # the blocks those handles freed into the library's cache: handed back to the device
    torch.cuda.synchronize()


def gpu(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def flags_of(D, names):
    out = 0
    for name in names:
        out |= getattr(D._lib, name)
    return out


# ---- handles and their M, built once per module ------------------------------------------------------------------------------------
_HANDLES, _APPLY, _WORST = {}, {}, {}


def handle(D, pc, name, reorder=None):
    key = (pc, name, reorder)
    if key not in _HANDLES:
        S = D.CsrSystem.from_any(C.matrix(name), reorder=reorder)
        assert S.reordered == (reorder is not None)
        S.set_preconditioner(C.make_preconditioner(D, pc))
        _HANDLES[key] = S
    return _HANDLES[key]


def device_hierarchy(S, A, pc):
    """The device's levels as the restatements' Hierarchy and smoothers (tests/test_amg_smoothers_gpu.py::_device)."""
    import amg_restatement as AR
    import amg_smoother_restatement as SR
    info = S.amg_hierarchy()
    assert info.precision == ("fp32" if pc == "amg_fp32" else "fp64")
    H, Al, colors = AR.Hierarchy(), C._canonical(A), []
    for l in range(info.levels - 1):
        lev = info.level(l)
        H.levels.append(AR.Level(Al, 1.0 / Al.diagonal(), lev.aggregates, lev.P, info.omega[l]))
        colors.append(lev.colors)
        Al = C._canonical(lev.A_next)
    H.levels.append(AR.Level(Al, 1.0 / Al.diagonal()))
    H.coarse_inv = np.linalg.inv(Al.toarray())
    kind = SR.GAUSS_SEIDEL if pc == "amg_gs" else SR.JACOBI
    assert info.levels >= 2 and info.smoother == [kind] * (info.levels - 1)
    return H, SR.smoothers_for(H, kind, rhos=info.rho, colorings=colors, kinds=info.smoother)


def factor_apply(S, pc, A):
    """M r from what the handle itself holds, in the caller's numbering."""
    kind = C.PCS[pc]["kind"]
    if kind in ("llt_multiply", "llt_solve"):
        rp, ci, v = S.factor()
        Lf = sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))
        return C.apply_llt_multiply(Lf) if kind == "llt_multiply" else C.apply_llt_solve(Lf)
    if kind in ("lu_multiply", "lu_solve"):
        Lf, Uf = S.lu_factors()
        return C.apply_lu_multiply(Lf, Uf) if kind == "lu_multiply" else C.apply_lu_solve(Lf, Uf)
    H, sm = device_hierarchy(S, A, pc)
    return C.apply_amg(pc, H, sm)


def apply_of(D, pc, name, reorder=None):
    key = (pc, name, reorder)
    if key not in _APPLY:
        _APPLY[key] = factor_apply(handle(D, pc, name, reorder), pc, C.matrix(name))
    return _APPLY[key]


# ---- which form a call takes, from the handle's own answers (the routing of dpcg_solve) -------------------------------------------
def form_of(D, S, flags=0, x_true=False):
    """"small" (one workgroup), "chip_llt", "chip_trsv" (whole chip), else the launches: "fused" (two-kernel updates) or "three_kernel"."""
    L = D._lib
    kind = S.info()["precond"]
    if kind == L.PRECOND_LLT_MULTIPLY and S.reduction_geometry()["small_threads"] > 0 and not x_true and not flags & (L.SPMV_F32 | L.NO_SMALL):
        return "small"
    if (kind in (L.PRECOND_LLT_MULTIPLY, L.PRECOND_LLT_SOLVE) and S.chip_info()["chip_by_default"] and not x_true
            and not flags & (L.SPMV_F32 | L.NO_TEAM | L.NO_FUSE | L.NO_SMALL | L.NO_GRAPH)):
        return "chip_llt" if kind == L.PRECOND_LLT_MULTIPLY else "chip_trsv"
    lossless = bool(flags & L.VAL32_IF_LOSSLESS)
    fused = S.info()["two_kernel_updates"] and not x_true and not flags & (L.NO_FUSE | L.SPMV_F32) and not lossless
    return "fused" if fused else "three_kernel"


def expected_form(case):
    """The form each case is meant to reach (sizes: driver_forms_cases' docstring)."""
    kind, launches = C.PCS[case.pc]["kind"], "NO_SMALL" in C.variant_kw(case.variant)["flags"]
    if not launches and kind == "llt_multiply":
        if case.system == "p79u":
            return "chip_llt"
        if case.reorder is None:
            return "small"
    return "fused"


def compare(case_id, group, res, ref, margin, moved, prefix, A, b, rtol_sq, atol_sq, count_allowed=True, prefix_rule=True):
    """The rule of the module's docstring.  count_allowed=False (DPCG_SPMV_F32 only: the issue's rule for it) and prefix_rule=False (that,
    and the fp32 V-cycle): the restatement rounds vectors to fp32 and is discontinuous in its input, so entries that happen to be stable
    under ONE perturbation need not be under another summation order."""
    diff = R.hist_diff(res.res_history, ref.history)
    count = R.is_count_case(margin, moved) and count_allowed
    true = R.true_residual(A, b, res.x.cpu().numpy())
    print(f"{case_id}: status {res.status} ({ref.status}), {res.iterations} updates (restatement {ref.updates}), margin {margin:.3f}, restatement moves "
          f"{moved:.2e} (stable prefix {prefix}), history differs by {diff:.3e}, true residual {true:.3e}, {'COUNT' if count else 'residual only'}")
    if case_id in C.COUNT_CASES and count_allowed:
        assert margin >= 1.2, f"the stop margin of this count case shrank to {margin:.3f}"
        assert moved < 1e-11, f"the restatement's own history moves by {moved:.2e}"
    if count:
        assert res.status == ref.status and res.iterations == ref.updates and len(res.res_history) == ref.updates + 1
        assert diff <= HIST_RTOL
        _WORST[group] = max(_WORST.get(group, 0.0), diff)
        if ref.status == R.MAX_ITER:
            np.testing.assert_allclose(res.x.cpu().numpy(), ref.x, rtol=1e-9, atol=1e-12)
        return count
    if ref.status == R.OK:
        thr = max(rtol_sq, atol_sq / float(b @ b))
        assert res.status == 0 and true < thr
        assert res.res_history[-1] < thr and (len(res.res_history) < 3 or res.res_history[1:-1].min() >= thr)
    else:
        assert res.status == ref.status and res.iterations == ref.updates and len(res.res_history) == ref.updates + 1
    if prefix_rule:
        k = min(prefix, len(res.res_history), len(ref.history))
        assert k >= 1 and R.hist_diff(res.res_history[:k], ref.history[:k]) <= HIST_RTOL, (case_id, k)
    return count


def group_of(pc):
    return next(g for g, pcs in C.GROUPS.items() if pc in pcs)


# ---- the matrix of cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.id)
def test_against_the_restatement(D, case):
    A, b, x0, _ = C.system(case.pc, case.system)
    S = handle(D, case.pc, case.system, case.reorder)
    v = C.variant_kw(case.variant, case.pc)
    flags = flags_of(D, v["flags"])
    assert form_of(D, S, flags) == expected_form(case), (S.info(), S.chip_info(), S.reduction_geometry())
    x0v, rtol_sq, atol_sq, cap, icr = C.solve_args(case)
    res = S.solve(gpu(b), None if x0v is None else gpu(x0v), rtol_sq=rtol_sq, atol_sq=atol_sq, max_iter=cap, flags=flags)
    assert res.recurrence == "standard"
    ref, margin, moved, prefix = C.classify(case, apply_of(D, case.pc, case.system, case.reorder))
    if case.variant.startswith("cap"):
        assert ref.status == R.MAX_ITER and res.status == D._lib.MAX_ITER and res.iterations == cap and len(res.res_history) == cap + 1
    if icr:
        # the first entry is <r,r>/<b,b> and not <z,z>/<b,b>: the two differ on this system, so the case can tell them apart
        z_first = C.reference(C.Case(case.pc, case.system, "x0"), apply_of(D, case.pc, case.system, case.reorder)).history[0]
        assert abs(ref.history[0] - z_first) > 1e-3 * ref.history[0]
        assert abs(res.res_history[0] - ref.history[0]) <= HIST_RTOL * ref.history[0]
    if case.variant == "atol":
        assert ref.status == R.OK                     # the absolute test is what ends it
    compare(case.id, group_of(case.pc), res, ref, margin, moved, prefix, A, b, rtol_sq, atol_sq, prefix_rule=case.pc != "amg_fp32")


def test_count_cases_and_forms_are_covered():
    """Conditions, not measurements: per preconditioner at least two thirds of the cases are count cases, and one per form."""
    assert C.NOT_COUNT_CASES <= {c.id for c in C.ALL_CASES} | C.GUESS_IDS
    seen = set()
    for group, pcs in C.GROUPS.items():
        cases = [c for pc in pcs for c in C.cases_of(pc)]
        count = [c for c in cases if c.id in C.COUNT_CASES]
        assert 3 * len(count) >= 2 * len(cases), (group, len(count), len(cases))
        forms, counted = {expected_form(c) for c in cases}, {expected_form(c) for c in count}
        assert forms == counted, (group, forms - counted)
        seen |= forms
    assert seen == {"small", "chip_llt", "fused"}
    print("largest history difference of the count cases that ran:", _WORST)


def test_triangular_solve_form_refuses_the_icholt_factor(D):
    """ICholT(1, 0.1) "solve" at 1 024 and 1 600 rows has the whole-chip triangular-solve form's shape, and the form refuses its factor
    (too many levels in natural order, rows too long with fill on the scattered system: the levels are asserted from S.info()): the plain
    call is the launches' bits (so the cases above ran what `expected_form` says), on a reordered handle too."""
    for name, reorder in (("w32x32", None), ("p40u", None), ("p40u", "rcm")):
        A, b, x0, _ = C.system("icholt_solve", name)
        S = handle(D, "icholt_solve", name, reorder)
        assert S.n >= 1024 and S.info()["precond"] == D._lib.PRECOND_LLT_SOLVE and not S.chip_info()["chip_by_default"]
        levels = S.info()["levels_lower"]
        assert levels == S.info()["levels_upper"] and (levels > 18 if name == "w32x32" else levels <= 16), (name, levels)
        one, launches = S.solve(gpu(b), gpu(x0)), S.solve(gpu(b), gpu(x0), flags=D._lib.NO_SMALL | D._lib.NO_TEAM)
        assert np.array_equal(one.res_history, launches.res_history) and torch.equal(one.x, launches.x)


# ---- launch flags, history, on the forms of one handle ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", list(C.PCS))
def test_launch_flags_are_bit_identical(D, pc, monkeypatch):
    """DPCG_NO_GRAPH against the replayed graph, DPCG_NO_FUSE (three kernels, deferred x, p2) against the two-kernel form,
    DPCG_DRIVER_ALTERNATE (singles and chunks mixed) and want_history=False: the same bits as the default launches on the same handle,
    to convergence and under caps that end a chunk midway -- and a fused solve after a DPCG_NO_FUSE one finds no stale p2."""
    L = D._lib
    name = C.PCS[pc]["systems"][-1]
    A, b, x0, _ = C.system(pc, name)
    S = handle(D, pc, name)
    base = L.NO_SMALL | L.NO_TEAM
    assert form_of(D, S, base) == "fused" and form_of(D, S, base | L.NO_FUSE) == "three_kernel"
    full = C.MULTIPLY_CAP if C.PCS[pc]["capped"] else 1024
    for max_iter in (full, 0, 1, 5, 7, 15):
        ref = S.solve(gpu(b), gpu(x0), flags=base, max_iter=max_iter)
        variants = [base | L.NO_GRAPH, base | L.NO_FUSE, base | L.NO_FUSE | L.NO_GRAPH, base]
        for i, fl in enumerate(variants):
            res = S.solve(gpu(b), gpu(x0), flags=fl, max_iter=max_iter)
            assert (res.status, res.iterations) == (ref.status, ref.iterations), (pc, max_iter, i)
            assert np.array_equal(res.res_history, ref.res_history), (pc, max_iter, i)
            assert torch.equal(res.x, ref.x) and res.final_res == ref.final_res, (pc, max_iter, i)
        monkeypatch.setenv("DPCG_DRIVER_ALTERNATE", "1")
        for fl in (base, base | L.NO_FUSE):
            alt = S.solve(gpu(b), gpu(x0), flags=fl, max_iter=max_iter)
            assert (alt.status, alt.iterations) == (ref.status, ref.iterations) and np.array_equal(alt.res_history, ref.res_history)
            assert torch.equal(alt.x, ref.x), (pc, max_iter, fl)
        monkeypatch.delenv("DPCG_DRIVER_ALTERNATE")
        for fl in (base, base | L.NO_FUSE, 0):
            with_h = ref if fl == base else S.solve(gpu(b), gpu(x0), flags=fl, max_iter=max_iter)
            bare = S.solve(gpu(b), gpu(x0), flags=fl, max_iter=max_iter, want_history=False)
            assert len(bare.res_history) == 0 and (bare.status, bare.iterations) == (with_h.status, with_h.iterations)
            assert torch.equal(bare.x, with_h.x), (pc, max_iter, fl)
    # each is also equal to the restatement: the default launches are (test_against_the_restatement), and these are their bits
    if form_of(D, S, 0) not in ("fused", "three_kernel"):
        one = S.solve(gpu(b), gpu(x0), max_iter=full)
        ref = S.solve(gpu(b), gpu(x0), flags=base, max_iter=full)
        assert not np.array_equal(one.res_history, ref.res_history), "other bits than the launches': it was the one-launch form"


# ---- error tracking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [None, "rcm"])
@pytest.mark.parametrize("pc", list(C.PCS))
def test_error_history(D, pc, reorder):
    """x_true (from a host sparse solve) against the restatement's err_history, on a plain and on a reordered handle (x_true is
    gathered like b); x_true keeps a system off every one-launch form -- shown by the bits: the solve equals the three-kernel launches'
    (DPCG_NO_SMALL | DPCG_NO_TEAM | DPCG_NO_FUSE) without x_true, which no one-launch form's do; it is refused together with DPCG_SPMV_F32."""
    name = C.PCS[pc]["systems"][-1]
    A, b, x0, x_true = C.system(pc, name)
    S = handle(D, pc, name, reorder)
    cap = 12 if C.PCS[pc]["kind"] != "amg" else 6
    case = C.Case(pc, name, f"cap{cap}", reorder)
    res = S.solve(gpu(b), gpu(x0), rtol_sq=C.CAP_RTOL_SQ, max_iter=cap, x_true=gpu(x_true))
    m = apply_of(D, pc, name, reorder)
    ref = C.reference(case, m, x_true=x_true)
    _, margin, moved, _ = C.classify(case, m)
    assert R.is_count_case(margin, moved), (margin, moved)
    assert res.status == D._lib.MAX_ITER and res.iterations == cap == ref.updates and len(res.err_history) == cap + 1
    e_diff = R.hist_diff(res.err_history, ref.err_history)
    print(f"{pc} {reorder}: err_history differs by {e_diff:.3e}, history by {R.hist_diff(res.res_history, ref.history):.3e}")
    assert R.hist_diff(res.res_history, ref.history) <= HIST_RTOL
    assert e_diff <= HIST_RTOL
    np.testing.assert_allclose(res.x.cpu().numpy(), ref.x, rtol=1e-9, atol=1e-12)
    # the launches without x_true: the same iterates (x_true adds kernels, it changes none)
    plain = S.solve(gpu(b), gpu(x0), rtol_sq=C.CAP_RTOL_SQ, max_iter=cap, flags=D._lib.NO_SMALL | D._lib.NO_TEAM | D._lib.NO_FUSE)
    assert plain.err_history is None and np.array_equal(plain.res_history, res.res_history) and torch.equal(plain.x, res.x)
    with pytest.raises(D._lib.DpcgError, match="x_true tracking is fp64 only") as e:
        S.solve(gpu(b), flags=D._lib.SPMV_F32, x_true=gpu(x_true))
    assert e.value.status == D._lib.ERR_INVALID


# ---- mixed precision ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", list(C.PCS))
def test_mixed_precision(D, pc):
    """DPCG_SPMV_F32 against the mixed restatement.  Rounding p to fp32 is discontinuous: the true residual, the last-but-one entry
    and |count - restatement| <= 1; the first entries, before anything is amplified, to the fp32 rounding of one p entry."""
    name = C.PCS[pc]["systems"][0]
    A, b, x0, _ = C.system(pc, name)
    S = handle(D, pc, name)
    case = C.Case(pc, name, "mixed")
    _, rtol_sq, atol_sq, cap, _ = C.solve_args(case)
    res = S.solve(gpu(b), rtol_sq=rtol_sq, max_iter=cap, flags=D._lib.SPMV_F32)
    ref, margin, moved, prefix = C.classify(case, apply_of(D, pc, name))
    compare(case.id, group_of(pc), res, ref, margin, moved, prefix, A, b, rtol_sq, atol_sq, count_allowed=False, prefix_rule=False)
    assert abs(res.iterations - ref.updates) <= 1
    plain = S.solve(gpu(b), rtol_sq=rtol_sq, max_iter=cap, flags=D._lib.NO_SMALL | D._lib.NO_TEAM)
    assert res.res_history[0] == plain.res_history[0] and not np.array_equal(res.res_history[:4], plain.res_history[:4])
    assert R.hist_diff(res.res_history[:4], ref.history[:4]) <= 1e-6


# ---- lossless fp32 values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", list(C.PCS))
def test_val32_if_lossless_is_bit_identical(D, pc):
    """The integer-valued 33x31 Poisson matrix is lossless in fp32: DPCG_VAL32_IF_LOSSLESS streams fp32 values and returns the bits of
    the plain three-kernel solve (the flag takes the two-kernel form away, include/dpcg.h)."""
    L = D._lib
    A, b, x0, _ = C.system(pc, "33x31")
    S = handle(D, pc, "33x31")
    base = L.NO_SMALL | L.NO_TEAM
    cap = C.MULTIPLY_CAP if C.PCS[pc]["capped"] else 1024
    first = S.solve(gpu(b), gpu(x0), flags=base | L.VAL32_IF_LOSSLESS, max_iter=cap)          # (decides "lossless" for the matrix)
    assert S.info()["two_kernel_updates"]                 # (what the flag takes away once the matrix is known to be lossless, as here)
    for extra in (0, L.NO_GRAPH):
        ref = S.solve(gpu(b), gpu(x0), flags=base | L.NO_FUSE | extra, max_iter=cap)
        res = S.solve(gpu(b), gpu(x0), flags=base | L.VAL32_IF_LOSSLESS | extra, max_iter=cap)
        assert (res.status, res.iterations) == (ref.status, ref.iterations) and np.array_equal(res.res_history, ref.res_history)
        assert torch.equal(res.x, ref.x) and torch.equal(first.x, ref.x)
    # a one-launch form keeps the matrix on chip in fp64: the flag does not keep the system off it, and changes no bit
    if form_of(D, S, 0) != "fused":
        a, c = S.solve(gpu(b), gpu(x0), max_iter=cap), S.solve(gpu(b), gpu(x0), flags=L.VAL32_IF_LOSSLESS, max_iter=cap)
        assert np.array_equal(a.res_history, c.res_history) and torch.equal(a.x, c.x)


# ---- the projected guess -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", list(C.PCS))
def test_projected_guess(D, pc):
    """guess=: three right-hand sides in sequence on one handle (driver_forms_cases.GuessRun).  The restatement's Guess is handed the
    DEVICE's solutions, so that its start vector for solve i is the one the device has to form.  Asserted for every solve, whatever
    its class: the device's start vector against the restatement's under the yardstick of tests/test_guess_gpu.py (8 x the distance of
    two sum orders), and the first history entry -- the start residual through M -- to 1e-10 where the restatement's is stable; then the
    solve from that start vector by the module's rule, its class named in COUNT_CASES like any other case."""
    name = C.PCS[pc]["systems"][0]
    S = handle(D, pc, name)
    run = C.GuessRun(pc, apply_of(D, pc, name))
    bar = C.guess_x0_yardstick()
    g = D.ProjectedGuess(S, depth=4)
    try:
        for i in range(C.GUESS_SOLVES):
            bi, x0, ref, margin, moved, prefix = run.step(i)
            x0_dev = g.project(gpu(bi)).cpu().numpy()                  # (solve() projects again: the same basis, the same bits)
            res = S.solve(gpu(bi), rtol_sq=C.RTOL_SQ, max_iter=run.cap, guess=g)
            if i == 0:
                assert not x0.any() and not x0_dev.any()
            else:
                dx = np.linalg.norm(x0_dev - x0) / np.linalg.norm(x0)
                print(f"{pc} guess {i}: x0 device-restatement {dx:.3e}, bar {bar:.3e}; first entry differs by "
                      f"{abs(res.res_history[0] - ref.history[0]) / ref.history[0]:.3e}")
                assert dx <= bar
                if not C.PCS[pc]["capped"]:
                    assert R.true_residual(run.A, bi, x0) < 0.5            # (the guess is a start vector that helps)
            if prefix >= 1:
                assert abs(res.res_history[0] - ref.history[0]) <= HIST_RTOL * ref.history[0]
            compare(C.guess_id(pc, i), group_of(pc), res, ref, margin, moved, prefix, run.A, bi, C.RTOL_SQ, 0.0,
                    count_allowed=pc != "amg_fp32", prefix_rule=pc != "amg_fp32")
            if pc == "amg_fp32":
                # the fp32 cycle rounds its vectors: as with DPCG_SPMV_F32, one rounding that falls the other way under the device's
                # summation order is amplified over the solve, whatever ONE perturbation of the restatement shows (measured: 4e-8 on
                # the history of a solve whose restatement moved by 5e-13) -- the residual rule, and the count within one
                assert abs(res.iterations - ref.updates) <= 1
            run.feed(res.x.cpu().numpy())
            assert g.info()["size"] == run.guesses["sequential"].size == i + 1
    finally:
        g.close()


# ---- update_values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", list(C.PCS))
def test_update_values_then_reattach(D, pc):
    """Scaled and drifted values on the same pattern, the preconditioner attached again, then a solve with x0: the bits of a fresh
    handle's, in every form -- neither the captured graph nor the fp32 copy of the values (one DPCG_SPMV_F32 solve runs before the
    update) is stale."""
    L = D._lib
    name = C.PCS[pc]["systems"][-1]
    A, b, x0, _ = C.system(pc, name)
    drift = 1.0 + 0.2 * np.random.default_rng(4).random(A.shape[0])
    A2 = C._canonical(1.5 * (sp.diags(drift) @ A @ sp.diags(drift)))
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(A2.indptr, A.indptr)
    cap = C.MULTIPLY_CAP if C.PCS[pc]["capped"] else 1024
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(C.make_preconditioner(D, pc))
    base = L.NO_SMALL | L.NO_TEAM
    for fl in (0, base, base | L.NO_FUSE, L.SPMV_F32):
        S.solve(gpu(b), gpu(x0), flags=fl, max_iter=cap)          # (captures the graphs, makes the fp32 copy of the OLD values)
    S.update_values(A2.data)
    assert S.info()["precond"] == 0
    S.set_preconditioner(C.make_preconditioner(D, pc))
    F = D.CsrSystem.from_any(A2, reorder=None)
    F.set_preconditioner(C.make_preconditioner(D, pc))
    for fl in (0, base, base | L.NO_FUSE, L.SPMV_F32, base | L.NO_GRAPH):
        assert form_of(D, S, fl) == form_of(D, F, fl)
        rs, rf = S.solve(gpu(b), gpu(x0), flags=fl, max_iter=cap), F.solve(gpu(b), gpu(x0), flags=fl, max_iter=cap)
        assert (rs.status, rs.iterations) == (rf.status, rf.iterations), (pc, fl)
        assert np.array_equal(rs.res_history, rf.res_history) and torch.equal(rs.x, rf.x), (pc, fl)
    # ... and it is the solve of the NEW system
    ref = R.pcg(A2, b, factor_apply(S, pc, A2), x0=x0, rtol_sq=C.RTOL_SQ, max_iter=min(cap, 10))
    res = S.solve(gpu(b), gpu(x0), flags=base, max_iter=min(cap, 10))
    if pc != "amg_fp32":
        assert R.hist_diff(res.res_history, ref.history[: len(res.res_history)]) <= HIST_RTOL
    S.close()
    F.close()


# ---- the forms one after the other on one handle, with AMG ------------------------------------------------------------------------
def test_forms_in_sequence_on_one_handle_with_amg(D, monkeypatch):
    """The graph, p2 and the chunk size are per-handle state: every form after every other one on ONE handle with AMG attached equals
    the same solve on a fresh handle, bit for bit."""
    L = D._lib
    A, b, x0, x_true = C.system("amg", "w32x32")
    base = L.NO_SMALL | L.NO_TEAM
    forms = [dict(flags=0), dict(flags=base | L.NO_FUSE), dict(flags=L.NO_GRAPH), dict(flags=L.SPMV_F32), dict(flags=0, x_true=True),
             dict(flags=base | L.NO_FUSE, max_iter=5), dict(flags=0, max_iter=3), dict(flags=L.VAL32_IF_LOSSLESS), dict(flags=L.INIT_CHECK_R)]

    def run(S, f):
        kw = dict(flags=f["flags"], max_iter=f.get("max_iter", 1024))
        if f.get("x_true"):
            kw["x_true"] = gpu(x_true)
        return S.solve(gpu(b), gpu(x0), **kw)

    alone = []
    for f in forms:
        F = D.CsrSystem.from_any(A, reorder=None)
        F.set_preconditioner(D.SmoothedAggregation())
        alone.append(run(F, f))
        F.close()
    n = len(forms)
    order = [i for u in range(n) for v in range(u + 1, n) for i in (u, v, u)]          # every pair, in both orders
    assert {(u, v) for u, v in zip(order, order[1:]) if u != v} == {(u, v) for u in range(n) for v in range(n) if u != v}
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.SmoothedAggregation())
    for step, k in enumerate(order):
        res, ref = run(S, forms[k]), alone[k]
        assert (res.status, res.iterations) == (ref.status, ref.iterations), (step, k)
        assert np.array_equal(res.res_history, ref.res_history), (step, k, int(np.argmax(res.res_history != ref.res_history)))
        assert torch.equal(res.x, ref.x), (step, k)
        if ref.err_history is not None:
            assert np.array_equal(res.err_history, ref.err_history), (step, k)
    S.close()
