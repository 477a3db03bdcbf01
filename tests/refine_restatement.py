"""numpy restatement of the mixed-precision PCG of dpcg_solve_refined (include/dpcg.h, "mixed-precision PCG"): fp32 STORAGE, fp64
arithmetic.  Every product and sum is formed in fp64; a value is rounded with np.float32 exactly where the device stores it to an
fp32 vector, and the dots run over the stored values.

    A32 = fl32(A values), dinv32 = fl32(1/a_ii);  bb = <b,b>;  x = x0 or 0;  total = 0
    outer s = 0, 1, ...:
        r = b - A x;  rr = <r,r>;  outer_history[s] = rr / bb
        stop OK if rr/bb < rtol_sq or rr < atol_sq;  MAX_ITER if total == max_iter or s == max_outer;  BREAKDOWN if rr (or rr/bb) is not
        finite;  MAX_ITER ("stagnated") if s >= 1 and rr >= 0.25 rr_prev
        sigma = sqrt(rr);  r32 = fl32(r / sigma);  target = max(inner_rtol_sq, 0.25 rtol_sq bb / rr)
        inner PCG on A32 d = r32 from d = 0, first test on <r,r>, test <r,r> / <r32,r32> < target, at most max_iter - total updates
        total += updates;  x += sigma d

The device sums in another order (wave trees, per-workgroup partials), so its fp64 alpha and beta differ in the last bits and an fp32
rounding can flip: inner histories agree only loosely.  `reverse` sums every dot back to front -- one of the perturbations the count
margin of test_refine_gpu.py is measured with.
"""

import numpy as np
import scipy.sparse as sp

from deflation_restatement import poisson, shifted_laplacian, true_residual  # noqa: F401  (re-exported for the tests)
from nullspace_restatement import BREAKDOWN, MAX_ITER, OK  # noqa: F401

f32 = np.float32


def _dot(a, b, reverse):
    # np.float64, not float: x / 0 is inf or NaN as on the device (under np.errstate), where a Python float would raise
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.float64(a[::-1] @ b[::-1]) if reverse else np.float64(a @ b)


def rounded_matrix(A):
    """A with every value rounded to fp32 (held in fp64: products with it are fp64 products of fp32 values)."""
    A32 = sp.csr_matrix(A, copy=True)
    with np.errstate(over="ignore"):
        A32.data = A32.data.astype(f32).astype(np.float64)
    return A32


def first_overflow(A, jacobi=False):
    """What the device refuses: ("matrix value", k) / ("reciprocal diagonal entry", i) of the first entry that is not finite in fp32."""
    with np.errstate(over="ignore", divide="ignore"):
        bad = np.flatnonzero(~np.isfinite(A.data.astype(f32)))
        if bad.size:
            return "matrix value", int(bad[0])
        if jacobi:
            bad = np.flatnonzero(~np.isfinite((1.0 / A.diagonal()).astype(f32)))
            if bad.size:
                return "reciprocal diagonal entry", int(bad[0])
    return None


def inner_pcg(A32, r32, dinv32, target, cap, reverse=False):
    """The fp32-stored PCG.  Returns (updates, d, hist): hist[t] = <r,r>_t / <r32,r32>, hist[0] = 1."""
    n = r32.shape[0]
    d = np.zeros(n, dtype=f32)
    r = r32.copy()

    def apply_m(v):
        return v.copy() if dinv32 is None else (dinv32.astype(np.float64) * v.astype(np.float64)).astype(f32)

    z = apply_m(r)
    p = z.copy()
    rho = _dot(r, z, reverse)
    bb = _dot(r, r, reverse)
    hist = [bb / bb]
    k = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        stop = hist[0] < target or not hist[0] == hist[0]
        while not stop and k < cap:
            q = (A32 @ p.astype(np.float64)).astype(f32)
            alpha = rho / _dot(p, q, reverse)
            d = (d.astype(np.float64) + alpha * p.astype(np.float64)).astype(f32)
            r = (r.astype(np.float64) - alpha * q.astype(np.float64)).astype(f32)
            z = apply_m(r)
            rho_new = _dot(r, z, reverse)
            p = (z.astype(np.float64) + (rho_new / rho) * p.astype(np.float64)).astype(f32)
            rho = rho_new
            k += 1
            res = _dot(r, r, reverse) / bb
            hist.append(res)
            stop = res < target or not res == res
    return k, d, np.array(hist)


def _inner_margin(hist, target, capped):
    """smallest distance (a factor >= 1 is "clear") of the inner tests from their threshold"""
    before = min(hist[:-1]) / target if len(hist) > 1 else np.inf
    return before if capped else min(before, target / hist[-1])


def solve_refined(A, b, x0=None, jacobi=False, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, inner_rtol_sq=1e-6, max_outer=16,
                  reverse=False):
    """Returns a dict: status, x, iterations, outer_steps, inner_counts (one per inner solve), res_history (iterations + 1 entries, as
    the device documents it), outer_history, final_res, reason ("" / "stagnated" / "cap" / "max_outer"), outer_margins and
    inner_margins (tested quantity / threshold or its inverse, whichever is >= 1 when the test is clear of its threshold)."""
    if max_iter < 0 or not inner_rtol_sq > 0 or max_outer < 1:
        raise ValueError("invalid argument")
    bad = first_overflow(A, jacobi)
    if bad is not None:
        raise ValueError(f"{bad[0]} {bad[1]} is not finite after rounding to fp32")
    b = np.asarray(b, dtype=np.float64)
    A32 = rounded_matrix(A)
    dinv32 = (1.0 / A.diagonal()).astype(f32) if jacobi else None
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    bb = _dot(b, b, reverse)
    total, s, rr_prev = 0, 0, 0.0
    status, reason = MAX_ITER, ""
    res_hist, outer_hist, counts, outer_margins, inner_margins = [], [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        while True:
            r = b - A @ x if (s > 0 or x0 is not None) else b.copy()
            rr = _dot(r, r, reverse)
            res = rr / bb
            outer_hist.append(res)
            if s == 0:
                res_hist.append(res)
            if res < rtol_sq or rr < atol_sq:
                status = OK
                outer_margins.append(max(rtol_sq / res if res > 0 else np.inf, atol_sq / rr if rr > 0 else (np.inf if atol_sq > 0 else 0.0)))
                break
            if total == max_iter or s == max_outer:
                reason = "cap" if total == max_iter else "max_outer"
                break
            if not np.isfinite(rr) or not res == res:
                status = BREAKDOWN
                break
            margin = res / rtol_sq
            if atol_sq > 0:
                margin = min(margin, rr / atol_sq)
            if s >= 1:
                if rr >= 0.25 * rr_prev:
                    reason = "stagnated"
                    break
                margin = min(margin, 0.25 * rr_prev / rr)
            outer_margins.append(margin)
            rr_prev = rr
            sigma = np.sqrt(rr)
            r32 = (r / sigma).astype(f32)
            target = max(inner_rtol_sq, 0.25 * rtol_sq * bb / rr)
            cap = max_iter - total
            k, d, hist = inner_pcg(A32, r32, dinv32, target, cap, reverse)
            if hist[-1] == hist[-1]:
                inner_margins.append(_inner_margin(hist, target, capped=not hist[-1] < target))
            res_hist.extend(hist[1:] * _dot(r32, r32, reverse) * rr / bb)
            counts.append(k)
            total += k
            x = x + sigma * d.astype(np.float64)
            s += 1
    return {"status": status, "x": x, "iterations": total, "outer_steps": s, "inner_counts": counts, "res_history": np.array(res_hist),
            "outer_history": np.array(outer_hist), "final_res": outer_hist[-1], "reason": reason, "outer_margins": outer_margins,
            "inner_margins": inner_margins}


def residual_bound(A, b, x, rr):
    """How far an fp64 evaluation of <r,r>, r = b - A x, may lie from another one: each r_i carries an error of at most
    n eps (|A||x| + |b|)_i whatever the order of its sum, so |delta rr| <= 2 sqrt(rr) n eps || |A||x| + |b| ||_2 to first order."""
    n = A.shape[0]
    w = abs(A) @ np.abs(x) + np.abs(b)
    return 2.0 * np.sqrt(rr) * n * np.finfo(np.float64).eps * np.linalg.norm(w)
