"""What tests/test_refine_edges_gpu.py relies on, asserted on the CPU with the numpy restatement (tests/refine_restatement.py): that
the systems of tests/refine_edge_cases.py reach every lanes-per-row class and indexing edge of k_rf_spmv, that the tolerances of the
short runs are the measured ones, that a restatement with ONE dropped matrix entry lies far outside them, that every stop case is
decided clear of its threshold, and that the restatement itself is invariant under the power-of-two scalings."""

import numpy as np
import pytest

import refine_edge_cases as C
import refine_restatement as R


def test_every_lanes_per_row_class_and_indexing_edge_is_reached():
    seen = set()
    ones = 0
    for name in C.SYSTEMS:
        A, _ = C.system(name)
        tpr = C.lanes_per_row(A)
        assert tpr == C.TPR[name], (name, tpr, A.nnz / A.shape[0])
        seen.add(tpr)
        starts, length = A.indptr[:-1], np.diff(A.indptr)
        assert A.has_sorted_indices and np.all(length >= 1)
        if A.shape[0] > 2:                                                   # (tiny(2): rows of 2 entries start at 0 and 2)
            assert np.any(starts % 2 == 1) and np.any(starts % 2 == 0), name
        if name.startswith("banded_spd"):
            assert 0.4 <= np.mean(starts % 2 == 1) <= 0.6, name
        ones += int(np.sum(length == 1))
    assert seen == {2, 4, 8, 16, 32, 64}
    assert ones > 0
    A, _ = C.system("boundary_identity(12)")
    starts, length = A.indptr[:-1], np.diff(A.indptr)
    assert {int(s) % 2 for s in starts[length == 1]} == {0, 1}               # rows of one entry at odd and at even starts
    A, _ = C.system("hub(12, 97)")
    starts, length = A.indptr[:-1], np.diff(A.indptr)
    hub = int(np.argmax(length))
    assert length[hub] == 98 and starts[hub] % 2 == 1 and length[hub] > 12 * 2 * C.lanes_per_row(A)   # an odd start, 13 trips a lane
    assert {A.shape[0] % 4 for A in (C.system(f"tiny({n})")[0] for n in range(1, 9))} == {0, 1, 2, 3}
    assert np.any(C.system("with_stored_zeros(poisson2d(12))")[0].data == 0.0)


@pytest.mark.parametrize("name,pre,t", C.SHORT_CASES)
def test_short_run_is_one_inner_solve_and_its_tolerance_is_the_floor(name, pre, t):
    """twice the measured spread is below the floor, so the floor is the tolerance (refine_edge_cases.X_TOL_ULPS, HIST_TOL)"""
    A, b = C.system(name)
    run = C.short_run(name, pre, t)
    sx, sh, same = C.measure_spread(name, pre, t)
    print(f"{name} {pre} t={t}: spread of x {sx:.3g} ulp, of the history {sh:.3g}; status {run['status']}, {run['iterations']} updates, "
          f"{run['outer_steps']} outer steps")
    assert same
    assert 2.0 * sx <= C.X_TOL_ULPS and 2.0 * sh <= C.HIST_TOL
    if name == "tiny(1)" and t >= 2:
        # one row: the first update solves the fp32 problem exactly (<r,r> = 0 stops the inner solve), the second outer step converges
        assert (run["status"], run["iterations"], run["outer_steps"]) == (R.OK, 2, 2)
    else:
        assert (run["status"], run["iterations"], run["outer_steps"], run["reason"]) == (R.MAX_ITER, t, 1, "cap")
        assert np.array_equal(C.one_inner_solve(A, b, pre, t), run["x"])      # the helper the mutants go through is the same run
    assert len(run["res_history"]) == run["iterations"] + 1


# Measured (profiles/refine_edges.md): the smallest factor over the three mutants at t = 2, 3 is 13.1, on
# scaled_rows(banded_spd(130, 6, 3), -3, 3, 1) with M = I (the last entry of its widest row is a small one); none falls short.
MUTANT_EXCLUSIONS = {}


@pytest.mark.parametrize("pre", C.PRES)
@pytest.mark.parametrize("name", list(C.SYSTEMS))
def test_a_dropped_entry_lies_far_outside_the_tolerance(name, pre):
    assert len(MUTANT_EXCLUSIONS) <= 2
    A, _ = C.system(name)
    present = 0
    for which in C.MUTANTS:
        pos = C.mutant_position(A, which)
        if pos is None:
            # tiny(1): no odd start; tiny(2): no odd start, no row of odd length
            assert name in ("tiny(1)", "tiny(2)"), (name, which)
            continue
        present += 1
        factors = {t: C.mutant_factor(name, pre, t, which) for t in C.TS}
        print(f"{name} {pre}, {which} (entry {pos}): " + ", ".join(f"t={t}: {f:.3g}" for t, f in factors.items()))
        if (name, pre) in MUTANT_EXCLUSIONS:
            continue
        assert factors[2] >= 10.0 and factors[3] >= 10.0
    assert present >= 1


def test_mutant_positions_are_what_they_claim():
    A, _ = C.system("banded_spd(203, 12, 2)")
    ip, length = A.indptr, np.diff(A.indptr)
    last = C.mutant_position(A, C.MUTANTS[0])
    assert last + 1 in ip and length[np.searchsorted(ip, last + 1) - 1] == length.max()
    first = C.mutant_position(A, C.MUTANTS[1])
    assert first in ip and first % 2 == 1
    alone = C.mutant_position(A, C.MUTANTS[2])
    row = np.searchsorted(ip, alone + 1) - 1
    assert alone + 1 == ip[row + 1] and ip[row] % 2 == 0 and length[row] % 2 == 1
    Z, _ = C.system("with_stored_zeros(poisson2d(12))")
    assert all(Z.data[C.mutant_position(Z, w)] != 0 for w in C.MUTANTS)


@pytest.mark.parametrize("case", list(C.stop_cases()))
def test_stop_cases_are_decided_clear_of_their_thresholds(case):
    ref = C.stop_restated(case)
    A, b, x0, pre, kw = C.stop_inputs(case)
    start = np.zeros_like(b) if x0 is None else x0
    print(case, ref["status"], ref["iterations"], ref["outer_steps"], ref["reason"], ref["outer_margins"])
    assert all(m >= 1.2 for m in ref["outer_margins"])
    if case.startswith("atol_sq"):
        bb = float(b @ b)
        assert (ref["status"], ref["outer_steps"]) == (R.OK, 2) and ref["final_res"] * bb < kw["atol_sq"] and ref["final_res"] > 1e-300
        assert ref["outer_history"][1] * bb >= 1.2 * kw["atol_sq"]
    elif case.startswith("max_outer"):
        assert (ref["status"], ref["reason"], ref["outer_steps"]) == (R.MAX_ITER, "max_outer", kw["max_outer"])
        assert np.all(np.diff(ref["outer_history"]) < 0) and ref["final_res"] >= 1.2 * kw["rtol_sq"]       # progress at every step
    elif case.startswith("cap at the end"):
        count, before = C.first_inner(C.STOP_SYSTEM, pre)
        assert before >= 1.2                    # the inner solve cannot stop one update early, which alone would open a second one
        assert (ref["status"], ref["reason"], ref["iterations"], ref["outer_steps"]) == (R.MAX_ITER, "cap", count, 1)
        assert ref["inner_counts"] == [count] and ref["final_res"] >= 1.2 * kw["rtol_sq"]
    elif case.startswith("zero updates"):
        assert (ref["status"], ref["reason"], ref["iterations"], ref["outer_steps"]) == (R.MAX_ITER, "stagnated", 0, 1)
        assert np.array_equal(ref["x"], start) and len(ref["res_history"]) == 1
        assert ref["outer_history"][1] == ref["outer_history"][0]
    elif case.startswith("b = 0") or case.startswith("b with one NaN"):
        want = R.MAX_ITER if "max_iter = 0" in case else R.OK if "atol_sq > 0" in case else R.BREAKDOWN
        assert (ref["status"], ref["iterations"], ref["outer_steps"]) == (want, 0, 0)
        assert np.array_equal(ref["x"], start) and np.isnan(ref["final_res"])
    else:
        assert case == "fp32 rounds A to zero"
        assert not R.rounded_matrix(A).data.any() and R.first_overflow(A) is None
        assert R.first_overflow(A, jacobi=True) == ("reciprocal diagonal entry", 0)
        assert (ref["status"], ref["iterations"], ref["outer_steps"], ref["inner_counts"]) == (R.BREAKDOWN, 1, 1, [1])
        assert not np.isfinite(ref["x"]).any()


# Measured (profiles/refine_edges.md): whether the candidate ends "stagnated" after >= 1 productive outer step, its smallest outer
# margin and the margin of the stagnation test itself, rr / (0.25 rr_prev).
STAGNATION_EXPECTED = {"scaled_rows(poisson2d(12), -4, 4)": False,     # no outer step is productive: <r,r> grows, the cap ends it
                       "jumping((16, 16), 4, 1e8)": False,             # stagnated, but at outer step 1: <r,r> grew by 1.1e4
                       "anisotropic2d(16, 1e-6)": False,               # stagnated at outer step 4, but by a factor 1.18 only
                       "anisotropic2d(16, 1e-7)": True}                # outer step 4, margins >= 9.1, the stop by 3.1


@pytest.mark.parametrize("name", list(C.STAGNATION_CANDIDATES))
def test_stagnation_candidates(name):
    A, b, run = C.stagnation_run(name)
    margin = min(run["outer_margins"]) if run["outer_margins"] else 0.0
    print(f"{name}: {run['reason'] or 'converged'} after {run['outer_steps']} outer steps, {run['iterations']} updates; outer margins >= "
          f"{margin:.3g}, the stop itself {C.stagnation_margin(run):.3g}; outer history {run['outer_history']}")
    assert C.qualifies_as_stagnation(run) == STAGNATION_EXPECTED[name]
    if name == C.STAGNATION_CASE:
        assert run["status"] == R.MAX_ITER and np.isfinite(run["x"]).all()
        assert np.all(np.diff(run["outer_history"][:-1]) < 0)                 # every step before the last was productive
        for tag in C.PERTURBATIONS:                                           # the same stop under every perturbation
            bp, reverse = C.perturbed(b, tag)
            other = R.solve_refined(A, bp, rtol_sq=1e-30, max_iter=20000, reverse=reverse)
            assert (other["reason"], other["outer_steps"]) == ("stagnated", run["outer_steps"])


@pytest.mark.parametrize("pre", C.PRES)
def test_the_restatement_is_invariant_under_power_of_two_scalings(pre):
    """k = +-60 and m = +-200 as asked: no fp32 value of the inner solve goes denormal (r32 is scaled by sigma, A32 = 2^k fl32(A) is
    far inside fp32's range), so k was not shrunk."""
    A, b = C.system(C.SCALING_SYSTEM)
    base = C.scaling_restated(pre)
    assert base["status"] == R.OK and base["outer_steps"] >= 2
    for k, m in C.SCALINGS:
        run = R.solve_refined(A * 2.0 ** k, b * 2.0 ** m, jacobi=pre == "jacobi", **C.SCALING_KW)
        assert (run["status"], run["iterations"], run["outer_steps"]) == (base["status"], base["iterations"], base["outer_steps"])
        assert np.array_equal(run["x"], base["x"] * 2.0 ** (m - k))
        assert np.array_equal(run["res_history"], base["res_history"]) and np.array_equal(run["outer_history"], base["outer_history"])


def test_division_by_zero_follows_ieee():
    """the restatement's scalars are numpy's: 0/0 and x/0 give NaN and inf as on the device, where a Python float would raise"""
    A, b = C.system("tiny(5)")
    zero = R.solve_refined(A, np.zeros(5))
    assert zero["status"] == R.BREAKDOWN and np.isnan(zero["final_res"])
    k, d, hist = R.inner_pcg(R.rounded_matrix(1e-50 * A), b.astype(np.float32), None, 1e-6, 10)
    assert k == 1 and np.isnan(hist[-1]) and np.all(np.isinf(d))
