"""tests/driver_restatement.py pinned to what the project already trusts (no GPU): the C oracle's PCG and mixed-precision PCG
(oracle/pcg_oracle.c, itself pinned to the reference's outputs by tests/test_oracle_golden.py) and the plain loop of
tests/deflation_restatement.py."""

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import deflation_restatement as DR
import driver_restatement as R
from oracle import c_oracle as CO

HIST_RTOL = 1e-10          # the project's bar for two correct summation orders of one history (tests/test_gpu_parity.py)
RTOL_SQ = 1e-8
SYSTEMS = {"5x7": lambda: DR.poisson((5, 7)), "40x40": lambda: DR.poisson((40, 40)), "33x31": lambda: DR.poisson((33, 31)),
           "w32x32": lambda: DR.shifted_laplacian((32, 32), 3)}


def _system(name):
    A = SYSTEMS[name]()
    return A, np.random.default_rng(1).random(A.shape[0])


@pytest.mark.parametrize("name", ["5x7", "40x40"])
@pytest.mark.parametrize("start", ["zero", "x0"])
def test_jacobi_reproduces_the_oracle(name, start):
    A, b = _system(name)
    x0 = None if start == "zero" else np.random.default_rng(2).random(A.shape[0])
    dinv = 1.0 / A.diagonal()
    for init_check_r in (False, True):
        # a count can only be compared where the stop is not a coin toss between two summation orders: the first of these thresholds
        # that the restatement's own history clears by the project's margin of 1.2 (tests/nullspace_restatement.py::stop_margin)
        # (Jacobi PCG gains ~1.2 per update on these systems, so most thresholds fall within 1.2 of an entry)
        for rtol_sq in (RTOL_SQ, 3e-9, 1e-9, 3e-10, 1e-10, 3e-8, 1e-7):
            ref = R.pcg(A, b, R.jacobi(A), x0=x0, rtol_sq=rtol_sq, init_check_r=init_check_r)
            if R.stop_margin(ref.history, rtol_sq) >= 1.2:
                break
        assert R.stop_margin(ref.history, rtol_sq) >= 1.2
        _, it, hist, x = CO.pcg(A, b, "jacobi", dinv=dinv, x0=x0, rtol=rtol_sq, init_check="r" if init_check_r else "z")
        assert ref.status == R.OK and ref.updates == it and R.hist_diff(ref.history, hist) <= HIST_RTOL
        np.testing.assert_allclose(ref.x, x, rtol=1e-9, atol=1e-12)
        # the loop is the one of deflation_restatement.pcg(W=None): the same bits
        status, count, h2, x2 = DR.pcg(A, b, apply_m=DR.jacobi(A), x0=x0, rtol_sq=rtol_sq, init_check_r=init_check_r)
        assert (status, count) == (ref.status, ref.updates) and np.array_equal(h2, ref.history) and np.array_equal(x2, ref.x)
    # a cap ends both after the same updates, with the same iterate
    capped = R.pcg(A, b, R.jacobi(A), x0=x0, rtol_sq=RTOL_SQ, max_iter=7)
    _, it, hist, x = CO.pcg(A, b, "jacobi", dinv=dinv, x0=x0, rtol=RTOL_SQ, max_iter=7)
    assert capped.status == R.MAX_ITER and capped.updates == it == 7 and R.hist_diff(capped.history, hist) <= HIST_RTOL
    np.testing.assert_allclose(capped.x, x, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", ["33x31", "w32x32"])
def test_mixed_loop_reproduces_the_oracle(name):
    """Rounding p to fp32 is discontinuous, so a late update may differ between two summation orders: the capped run, where nothing
    has been amplified yet, is compared entry by entry, the converged one by its count (+-1) and its true residual."""
    A, b = _system(name)
    x0 = np.random.default_rng(2).random(A.shape[0])
    dinv = 1.0 / A.diagonal()
    for kw in (dict(), dict(x0=x0)):
        ref = R.pcg(A, b, R.jacobi(A), rtol_sq=RTOL_SQ, spmv=R.mixed_spmv(A), **kw)
        _, it, hist, x = CO.pcg(A, b, "jacobi", dinv=dinv, rtol=RTOL_SQ, mixed=True, **kw)
        assert ref.status == R.OK and abs(ref.updates - it) <= 1
        assert R.true_residual(A, b, ref.x) < 10 * RTOL_SQ            # (the recurrence's residual, not the true one, is what is tested)
        m = min(len(hist), len(ref.history), 9)
        assert R.hist_diff(ref.history[:m], hist[:m]) <= 1e-6          # one fp32 rounding of p flipped moves an entry by ~1e-7 at most
        plain = R.pcg(A, b, R.jacobi(A), rtol_sq=RTOL_SQ, **kw)
        assert not np.array_equal(plain.history[:m], ref.history[:m])  # (the hook is in the loop)
        assert plain.history[0] == ref.history[0]                      # (and only there: the start residual is fp64)


@pytest.mark.parametrize("name", ["33x31", "w32x32"])
def test_error_history_is_consistent_with_x(name):
    A, b = _system(name)
    x_true = spla.spsolve(A.tocsc(), b)
    x0 = np.random.default_rng(2).random(A.shape[0])
    for kw in (dict(), dict(x0=x0), dict(max_iter=5), dict(max_iter=0, x0=x0)):
        ref = R.pcg(A, b, R.jacobi(A), rtol_sq=RTOL_SQ, x_true=x_true, **kw)
        assert len(ref.err_history) == len(ref.history) == ref.updates + 1
        e = ref.x - x_true
        assert ref.err_history[-1] == e @ (A @ e)                                   # the definition, at the last iterate
        e0 = (np.zeros_like(b) if "x0" not in kw else x0) - x_true
        assert ref.err_history[0] == e0 @ (A @ e0)                                  # and at the start vector
        assert np.all(np.diff(ref.err_history) < 0)                                 # CG minimises exactly this quantity
        without = R.pcg(A, b, R.jacobi(A), rtol_sq=RTOL_SQ, **kw)
        assert without.err_history is None and np.array_equal(without.x, ref.x) and np.array_equal(without.history, ref.history)


def test_classification():
    A, b = _system("33x31")
    m = R.jacobi(A)
    ref = R.pcg(A, b, m, rtol_sq=RTOL_SQ)
    margin, moved, prefix = R.classify(A, b, ref, lambda b2: R.pcg(A, b2, m, rtol_sq=RTOL_SQ), RTOL_SQ)
    assert prefix == len(ref.history)
    assert R.stable_prefix([1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.1, 4.0]) == 2 and R.stable_prefix([1.0, 2.0], [1.0]) == 1
    assert margin == R.stop_margin(ref.history, RTOL_SQ) and moved < 1e-11 and R.is_count_case(margin, moved) == (margin >= 1.2)
    capped = R.pcg(A, b, m, rtol_sq=RTOL_SQ, max_iter=5)
    assert R.margin_of(capped, RTOL_SQ) == capped.history.min() / RTOL_SQ > 1.2
    assert R.margin_of(capped, 0.0) == np.inf
    # the absolute test in force: the margin is taken against atol_sq / <b,b>
    atol_sq = 1e-6 * (b @ b)
    ra = R.pcg(A, b, m, rtol_sq=0.0, atol_sq=atol_sq)
    assert ra.status == R.OK and ra.history[-1] < 1e-6 <= ra.history[-2]
    assert R.margin_of(ra, 0.0, atol_sq, b @ b) == pytest.approx(R.stop_margin(ra.history, 1e-6), rel=1e-12)
