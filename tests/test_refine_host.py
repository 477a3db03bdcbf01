"""The numpy restatement of the mixed-precision PCG (tests/refine_restatement.py) on its own: what test_refine_gpu.py relies on."""

import numpy as np
import pytest

import refine_cases as cases
import refine_restatement as R


@pytest.mark.parametrize("pre", ["identity", "jacobi"])
@pytest.mark.parametrize("name", list(cases.SYSTEMS))
def test_refinement_reaches_what_fp32_alone_cannot(name, pre):
    """(a) rtol_sq = 1e-20 is reached, as a recomputed true residual, in >= 2 outer steps; (b) the same inner PCG without the outer loop
    (max_outer = 1) does not reach it."""
    A, b = cases.system(name)
    out = cases.restated(name, pre, 1e-20)
    assert out["status"] == R.OK and out["outer_steps"] >= 2
    assert R.true_residual(A, b, out["x"]) < 1e-20
    assert out["final_res"] == out["outer_history"][-1] and np.all(np.diff(out["outer_history"]) < 0)
    assert len(out["res_history"]) == out["iterations"] + 1 and sum(out["inner_counts"]) == out["iterations"]
    one = R.solve_refined(A, b, jacobi=pre == "jacobi", rtol_sq=1e-20, max_iter=cases.MAX_ITER, max_outer=1)
    assert one["status"] == R.MAX_ITER and one["reason"] == "max_outer" and one["outer_steps"] == 1
    assert R.true_residual(A, b, one["x"]) > 1e-16


@pytest.mark.parametrize("name", list(cases.SYSTEMS))
def test_default_tolerance_takes_one_or_two_outer_steps(name):
    """(c)"""
    out = cases.restated(name, "jacobi", 1e-8)
    assert out["status"] == R.OK and out["outer_steps"] in (1, 2)


def test_edges_of_the_definition():
    """(d)"""
    A, b = cases.system("poisson 40x40")
    zero = R.solve_refined(A, b, max_iter=0)
    assert zero["status"] == R.MAX_ITER and zero["reason"] == "cap" and zero["iterations"] == 0 and zero["outer_steps"] == 0
    assert not zero["x"].any() and zero["final_res"] == 1.0
    x = cases.restated("poisson 40x40", "jacobi", 1e-20)["x"]
    done = R.solve_refined(A, b, x0=x, rtol_sq=1e-8)
    assert done["status"] == R.OK and done["iterations"] == 0 and done["outer_steps"] == 0 and np.array_equal(done["x"], x)
    capped = R.solve_refined(A, b, rtol_sq=1e-20, max_iter=80)           # the first inner solve takes 67 updates, the second is cut
    assert capped["status"] == R.MAX_ITER and capped["reason"] == "cap" and capped["iterations"] == 80
    assert capped["inner_counts"] == [67, 13] and capped["outer_steps"] == 2
    stalled = R.solve_refined(A, b, rtol_sq=1e-20, inner_rtol_sq=2.0)    # an inner solve that does nothing: the outer step stagnates
    assert stalled["status"] == R.MAX_ITER and stalled["reason"] == "stagnated" and stalled["iterations"] == 0
    for bad in ({"max_iter": -1}, {"inner_rtol_sq": 0.0}, {"max_outer": 0}):
        with pytest.raises(ValueError):
            R.solve_refined(A, b, **bad)


def test_overflow_is_named():
    A, b = cases.system("poisson 5x7")
    B = A.copy()
    B.data[7] = 1e39
    assert R.first_overflow(B) == ("matrix value", 7)
    with pytest.raises(ValueError, match="matrix value 7"):
        R.solve_refined(B, b)
    B = A.copy()
    B.data[B.indptr[3] + np.flatnonzero(B.indices[B.indptr[3]:B.indptr[4]] == 3)[0]] = 1e-39
    assert R.first_overflow(B, jacobi=True) == ("reciprocal diagonal entry", 3)
