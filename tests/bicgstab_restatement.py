"""numpy restatement of the right-preconditioned BiCGStab of dpcg_solve_bicgstab (include/dpcg.h, "BiCGStab"), statement by statement.

    r0 = b - A x0;  rhat = r0;  bb = <b,b>;  rho = alpha = omega = 1;  v = p = 0;  history[0] = <r0,r0>/bb, tested
    update k:  rho' = <rhat,r>;  beta = (rho'/rho)(alpha/omega);  rho = rho'
               p = r + beta (p - omega v);  ph = M p;  v = A ph;  alpha = rho / <rhat,v>
               s = r - alpha v;  ss = <s,s>
               if ss meets the test:  x += alpha ph;  history[k+1] = ss/bb;  count = k+1;  stop (0)
               sh = M s;  t = A sh;  omega = <t,s>/<t,t>
               x += alpha ph + omega sh;  r = s - omega t;  history[k+1] = <r,r>/bb;  test

`dot` is injectable: the default is numpy's pairwise sum of the products, `strided_dot` adds 256 strided partial sums one after the
other (the shape of a device reduction).  BiCGStab amplifies the difference between two such orders exponentially in the update count,
which is why the device tests compare whole histories only over the first K updates (test_bicgstab_host.py measures K) and hold the
runs to the solution to their count, their stopping margins and the true residual instead.  M is a callable v -> M v (None: identity).
No dot is contracted with a product: every statement is one rounding per operation, as the kernels are compiled (-ffp-contract=off).
"""

import numpy as np

OK, MAX_ITER, BREAKDOWN = 0, 1, 2


def plain_dot(a, b):
    return np.float64(np.sum(a * b))        # (np.float64, not float: 0/0 is then a NaN and not an exception)


def strided_dot(a, b, ways=256):
    """`ways` partial sums over the entries i, i + ways, ..., each in index order, added one after the other"""
    prod = a * b
    pad = (-prod.size) % ways
    lanes = np.add.reduce(np.concatenate([prod, np.zeros(pad)]).reshape(-1, ways), axis=0)   # row after row: x + 0.0 changes no bit
    tot = np.float64(0.0)
    for v in lanes:
        tot = tot + v
    return tot


def bicgstab(A, b, M=None, x0=None, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, dot=plain_dot):
    """-> dict(status, iterations, x, history).  A: anything with `@`; M: callable or None."""
    apply_m = (lambda v: v) if M is None else M
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x if x0 is not None else b.copy()
    rhat = r.copy()
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        rho = alpha = omega = np.float64(1.0)
        v = np.zeros_like(b)
        p = np.zeros_like(b)
        rr = dot(r, r)
        history = [rr / bb]

        def meets(q):
            return (q / bb < rtol_sq) or (q < atol_sq)

        def done(status, k):
            return {"status": status, "iterations": k, "x": x, "history": np.array(history)}

        k = 0
        while True:
            if meets(rr):
                return done(OK, k)
            if np.isnan(history[-1]):
                return done(BREAKDOWN, k)
            if k == max_iter:
                return done(MAX_ITER, k)
            rho_new = dot(rhat, r)
            if rho_new == 0.0 or not np.isfinite(rho_new):
                return done(BREAKDOWN, k)
            beta = (rho_new / rho) * (alpha / omega)
            rho = rho_new
            p = r + beta * (p - omega * v)
            ph = apply_m(p)
            v = A @ ph
            rv = dot(rhat, v)
            if rv == 0.0 or not np.isfinite(rv):
                return done(BREAKDOWN, k)
            alpha = rho / rv
            s = r - alpha * v
            ss = dot(s, s)
            if meets(ss):
                x = x + alpha * ph
                history.append(ss / bb)
                return done(OK, k + 1)
            sh = apply_m(s)
            t = A @ sh
            ts = dot(s, t)
            tt = dot(t, t)
            if tt == 0.0 or not (np.isfinite(tt) and np.isfinite(ts) and np.isfinite(ss)):
                return done(BREAKDOWN, k)
            omega = ts / tt
            x = (x + alpha * ph) + omega * sh
            r = s - omega * t
            rr = dot(r, r)
            history.append(rr / bb)
            k += 1


def stop_margin(history, rtol_sq=1e-8):
    """(history[-2] / rtol_sq, rtol_sq / history[-1]): how clear of the threshold the last two tested values are (both > 1 for a
    converged run; tests/nullspace_restatement.py::stop_margin is the model)"""
    before = history[-2] / rtol_sq if len(history) > 1 else np.inf
    return before, rtol_sq / history[-1]


def true_residual(A, b, x):
    e = b - A @ x
    return float(e @ e) / float(b @ b)


def rel_spread(a, b):
    """largest |a_k - b_k| / |b_k| of two histories, and the max-norm relative distance of two vectors, share this"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def x_spread(xa, xb):
    return float(np.max(np.abs(xa - xb)) / np.max(np.abs(xb)))
