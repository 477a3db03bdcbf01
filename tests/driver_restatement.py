"""numpy fp64 restatement of the plain PCG driver (dpcg_solve in include/dpcg.h) with the hooks the driver's solve forms need: the
loop and stopping rule of tests/deflation_restatement.py::pcg(W=None), plus

    spmv=     p -> "A p" of the LOOP (DPCG_SPMV_F32: fp32-stored values and fp32-stored p, `mixed_spmv` below).  Only that product is
              mixed -- the start residual b - A x0, <p, Ap> with the fp64 p, the updates, M and the tests stay fp64 (orc_pcg_mixed);
    x_true=   the error history of include/dpcg.h: err_history[k] = (x_k - x_true)^T A (x_k - x_true) with the fp64 A, one entry per
              history entry, entry 0 for the start vector (k_anorm_err forms e = x - x_true, a plain SpMV forms A e, k_record_err sums
              <e, A e> and stores it at the update count -- also for the iterate the stopping test fired on).

    start:   r = b - A x0 (x0 None: r = b);  z = M r;  p = z;  rho = <r,z>
             first test on <z,z>/<b,b> (init_check_r: <r,r>/<b,b>) against rtol_sq, and on <z,z> (<r,r>) against atol_sq
    update:  q = spmv(p);  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  z = M r;  rho' = <r,z>;  p = z + (rho'/rho) p
             test: <r,r>/<b,b> < rtol_sq or <r,r> < atol_sq;  a NaN ends the loop as a breakdown;  at most max_iter updates

`classify` is the rule of tests/test_deflation_gpu.py by which a device solve is compared with this loop (count and history, or the
true residual only), extended to capped solves.
"""

from dataclasses import dataclass

import numpy as np

from nullspace_restatement import BREAKDOWN, MAX_ITER, OK, jacobi, stop_margin  # noqa: F401  (re-exported: one definition)


@dataclass
class Result:
    status: int
    updates: int
    history: np.ndarray
    x: np.ndarray
    err_history: "np.ndarray | None" = None


def mixed_spmv(A):
    """p -> fp64(fp32(A)) fp64(fp32(p)), products and row sums in fp64: the project's statement of that product (orc_spmv_mixed)."""
    from oracle import c_oracle as CO
    return lambda p: CO.spmv_mixed(A, p)


def pcg(A, b, apply_m=None, x0=None, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, init_check_r=False, spmv=None, x_true=None):
    """apply_m: r -> M r (None: M = I).  spmv: p -> A p of the loop (None: the fp64 A)."""
    m = (lambda r: r.copy()) if apply_m is None else apply_m
    mul = (lambda p: A @ p) if spmv is None else spmv
    b = np.asarray(b, dtype=np.float64)
    if x0 is None:
        x = np.zeros_like(b)
        r = b.copy()
    else:
        x = np.array(x0, dtype=np.float64)
        r = b - A @ x
    err = None if x_true is None else []

    def record(xk):
        if err is not None:
            e = xk - x_true
            err.append(e @ (A @ e))

    bb = b @ b
    z = m(r)
    p = z.copy()
    rho = r @ z
    hist = []
    with np.errstate(divide="ignore", invalid="ignore"):
        first = r @ r if init_check_r else z @ z
        res = first / bb
        hist.append(res)
        record(x)
        status, k = MAX_ITER, 0
        if res < rtol_sq or first < atol_sq:
            status = OK
        elif not res == res:
            status = BREAKDOWN
        while status == MAX_ITER and k < max_iter:
            q = mul(p)
            alpha = rho / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            z = m(r)
            rho_new = r @ z
            p = z + (rho_new / rho) * p
            rho = rho_new
            k += 1
            rr = r @ r
            res = rr / bb
            hist.append(res)
            record(x)
            if res < rtol_sq or rr < atol_sq:
                status = OK
            elif not res == res:
                status = BREAKDOWN
    return Result(status, k, np.array(hist), x, None if err is None else np.array(err))


def true_residual(A, b, x):
    """||b - A x||^2 / ||b||^2"""
    e = b - A @ x
    return (e @ e) / (b @ b)


def hist_diff(dev, ref):
    """The largest relative difference of two histories (inf: their lengths differ)."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    return float(np.max(np.abs(dev - ref) / np.abs(ref))) if len(dev) == len(ref) else np.inf


def margin_of(ref: Result, rtol_sq, atol_sq=0.0, bb=1.0):
    """How far the tested quantity stays from the threshold that ends (or could end) the solve.  A converged solve: `stop_margin`
    (against atol_sq / <b,b> when the absolute test is the one in force).  A capped solve (MAX_ITER): the smallest entry over the
    threshold -- no entry may come within the margin of stopping the solve early.  No threshold at all: inf."""
    thr = max(rtol_sq, atol_sq / bb)
    if not thr > 0.0:
        return np.inf
    if ref.status == OK:
        return stop_margin(ref.history, thr)
    return float(np.min(ref.history)) / thr


def stable_prefix(hist, perturbed, bar=1e-11):
    """How many leading entries of a history move by less than `bar`, relatively, under the perturbation -- every one of them, up to
    the first that does not (or to the shorter of the two)."""
    m = min(len(hist), len(perturbed))
    moved = np.abs(np.asarray(perturbed[:m]) - np.asarray(hist[:m])) / np.abs(np.asarray(hist[:m]))
    bad = np.nonzero(~(moved < bar))[0]
    return int(bad[0]) if bad.size else m


def classify(A, b, ref: Result, rerun, rtol_sq, atol_sq=0.0):
    """(margin, moved, prefix): the reference's margin, how far its own history moves, relatively, when b is perturbed by 1e-16
    relative (`rerun(b2)` solves the same case for the right-hand side b2; inf: the count moved), and how many leading entries move
    by less than 1e-11 each.  A COUNT case has margin >= 1.2 and moved < 1e-11: only then do count and history of a correct device
    solve have to agree with the restatement; any other case still has to agree with it over the stable prefix."""
    b2 = b + 1e-16 * np.abs(b).max() * np.random.default_rng(9).standard_normal(b.size)
    h2 = rerun(b2).history
    return margin_of(ref, rtol_sq, atol_sq, float(b @ b)), hist_diff(h2, ref.history), stable_prefix(ref.history, h2)


def is_count_case(margin, moved):
    return margin >= 1.2 and moved < 1e-11
