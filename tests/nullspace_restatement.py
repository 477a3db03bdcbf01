"""numpy fp64 restatement of PCG with a null-space projection (include/dpcg.h, "singular systems"), with the project's stopping
rule: the first test on <p0,p0>/<b',b'> (or <r0,r0>/<b',b'> with init_check_r), then <r,r>/<b',b'> < rtol_sq or <r,r> < atol_sq
after every update, a NaN ends the loop as a breakdown, at most max_iter updates.

    b' = P b;  r = b' - A x0 (x0 given: r = P r once);  zt = M r;  s = Z^T zt;  t = Z^T r;  rho = <r,zt> - t^T s;  p = zt - Z s
    update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  zt = M r;  s = Z^T zt;  t = Z^T r
             rho' = <r,zt> - t^T s;  p = (zt - Z s) + (rho'/rho) p
    end:     x = x - Z (Z^T x)

Z = None runs the same loop without any projection (plain PCG): what a handle without a null space does.
"""

import numpy as np

OK, MAX_ITER, BREAKDOWN = 0, 1, 2


def orthonormalise(Z):
    """fp64 modified Gram-Schmidt, every column orthogonalised twice; ValueError for a rank-deficient Z (a column's norm after
    orthogonalisation below 1e-12 of its norm before)."""
    Q = np.array(Z, dtype=np.float64, order="F", copy=True)
    if Q.ndim == 1:
        Q = Q.reshape(-1, 1)
    for j in range(Q.shape[1]):
        before = np.linalg.norm(Q[:, j])
        for _ in range(2):
            for i in range(j):
                Q[:, j] -= (Q[:, i] @ Q[:, j]) * Q[:, i]
        after = np.linalg.norm(Q[:, j])
        if not after > 1e-12 * before:
            raise ValueError(f"rank deficient: column {j}")
        Q[:, j] /= after
    return Q


def constant(n):
    return np.full((n, 1), 1.0 / np.sqrt(n))


def project(Z, v):
    return v if Z is None else v - Z @ (Z.T @ v)


def pcg(A, b, Z, apply_m=None, x0=None, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, init_check_r=False):
    """Returns (status, updates, history, x).  apply_m: r -> M r (None: M = I).  Z: orthonormal (n, k), or None."""
    m = (lambda r: r.copy()) if apply_m is None else apply_m
    k_cols = 0 if Z is None else Z.shape[1]
    zt_dot = (lambda v: np.zeros(0)) if Z is None else (lambda v: Z.T @ v)
    z_times = (lambda c: 0.0) if Z is None else (lambda c: Z @ c)
    bp = project(Z, np.asarray(b, dtype=np.float64))
    if x0 is None:
        x = np.zeros_like(bp)
        r = bp.copy()
    else:
        x = np.array(x0, dtype=np.float64)
        r = project(Z, bp - A @ x)
    bb = bp @ bp
    zt = m(r)
    s, t = zt_dot(zt), zt_dot(r)
    rho = r @ zt - (t @ s if k_cols else 0.0)
    p = zt - z_times(s)
    hist = []
    with np.errstate(divide="ignore", invalid="ignore"):
        first = r @ r if init_check_r else zt @ zt - (s @ s if k_cols else 0.0)
        res = first / bb
        hist.append(res)
        status, k = MAX_ITER, 0
        if res < rtol_sq or first < atol_sq:
            status = OK
        elif not res == res:
            status = BREAKDOWN
        while status == MAX_ITER and k < max_iter:
            q = A @ p
            alpha = rho / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            zt = m(r)
            s, t = zt_dot(zt), zt_dot(r)
            rho_new = r @ zt - (t @ s if k_cols else 0.0)
            p = (zt - z_times(s)) + (rho_new / rho) * p
            rho = rho_new
            k += 1
            rr = r @ r
            res = rr / bb
            hist.append(res)
            if res < rtol_sq or rr < atol_sq:
                status = OK
            elif not res == res:
                status = BREAKDOWN
    return status, k, np.array(hist), project(Z, x)


def jacobi(A):
    dinv = 1.0 / A.diagonal()
    return lambda r: dinv * r


def true_residual(A, b, Z, x):
    """||P b - A x||^2 / ||P b||^2"""
    bp = project(Z, np.asarray(b, dtype=np.float64))
    e = bp - A @ x
    return (e @ e) / (bp @ bp)


def stop_margin(hist, rtol_sq=1e-8):
    """How far the tested quantity stays from the threshold: the smallest of hist[k] / rtol_sq over the entries before the stop
    and of rtol_sq / hist[-1] at it (both > 1 for a converged history; 1.2 is what a count comparison across summation orders
    needs by a wide margin -- the orders differ by ~1e-13 relative)."""
    before = min(hist[:-1]) / rtol_sq if len(hist) > 1 else np.inf
    return min(before, rtol_sq / hist[-1])
