"""numpy fp64 restatement of deflated PCG (include/dpcg.h, "deflated PCG"; Saad, Yeung, Erhel, Guyomarc'h, SISC 21, 2000) with the
project's stopping rule: the first test on <z0,z0>/<b,b> (or <r0,r0>/<b,b> with init_check_r) on the r AFTER the start correction,
then <r,r>/<b,b> < rtol_sq or <r,r> < atol_sq after every update, a NaN ends the loop as a breakdown, at most max_iter updates.

    start:   r = b - A x0 (x0 None: r = b);  c = W^T r;  x = x0 + W c;  r = r - AW c;  z = M r;  mu = AW^T z;  p = z - W mu;  rho = <r,z>
    update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  z = M r;  mu = AW^T z;  rho' = <r,z>
             p = (z - W mu) + (rho'/rho) p

W, AW: A-orthonormal (W^T A W = I) with AW = A W, as `a_orthonormalise` or the device's dpcg_get_deflation give them.  W = None runs
the same loop without deflation (plain PCG): what a handle without a deflation does.
"""

import numpy as np

from nullspace_restatement import BREAKDOWN, MAX_ITER, OK, jacobi, stop_margin  # noqa: F401  (re-exported: one definition)

TOL_DEP = 1e-7


def a_orthonormalise(A, W):
    """CholQR2 in the A inner product: AW = A W, then twice G = W^T AW, G = R^T R, W <- W R^-1, AW <- AW R^-1.  ValueError names a
    dependent column: a pivot <= TOL_DEP^2 G_jj."""
    W = np.array(W, dtype=np.float64, order="F", copy=True)
    if W.ndim == 1:
        W = W.reshape(-1, 1)
    AW = np.asfortranarray(A @ W)
    k = W.shape[1]
    for _ in range(2):
        G = W.T @ AW
        R = np.zeros((k, k))
        for j in range(k):
            p = G[j, j] - R[:j, j] @ R[:j, j]
            if not np.isfinite(p) or not p > TOL_DEP ** 2 * G[j, j]:
                raise ValueError(f"dependent: column {j}")
            R[j, j] = np.sqrt(p)
            for m in range(j + 1, k):
                R[j, m] = (G[j, m] - R[:j, j] @ R[:j, m]) / R[j, j]
        T = np.linalg.inv(R)
        W, AW = W @ T, AW @ T
    return W, AW


def pcg(A, b, W=None, AW=None, apply_m=None, x0=None, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, init_check_r=False):
    """Returns (status, updates, history, x).  apply_m: r -> M r (None: M = I)."""
    m = (lambda r: r.copy()) if apply_m is None else apply_m
    b = np.asarray(b, dtype=np.float64)
    if x0 is None:
        x = np.zeros_like(b)
        r = b.copy()
    else:
        x = np.array(x0, dtype=np.float64)
        r = b - A @ x
    if W is not None:
        c = W.T @ r
        x = x + W @ c
        r = r - AW @ c
    bb = b @ b
    z = m(r)
    p = z if W is None else z - W @ (AW.T @ z)
    rho = r @ z
    hist = []
    with np.errstate(divide="ignore", invalid="ignore"):
        first = r @ r if init_check_r else z @ z
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
            z = m(r)
            rho_new = r @ z
            zd = z if W is None else z - W @ (AW.T @ z)
            p = zd + (rho_new / rho) * p
            rho = rho_new
            k += 1
            rr = r @ r
            res = rr / bb
            hist.append(res)
            if res < rtol_sq or rr < atol_sq:
                status = OK
            elif not res == res:
                status = BREAKDOWN
    return status, k, np.array(hist), x


def true_residual(A, b, x):
    """||b - A x||^2 / ||b||^2"""
    e = b - A @ x
    return (e @ e) / (b @ b)


def shifted_laplacian(dims, seed, shift=0.05):
    """The seeded edge-weighted graph Laplacian of a dims grid (poisson.neumann_csr) plus shift * I: symmetric positive definite."""
    import scipy.sparse as sp
    from deeppreconditioning_amd.poisson import neumann_csr
    A = sp.csr_matrix(neumann_csr(dims, seed) + shift * sp.identity(int(np.prod(dims)), format="csr"))
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


def poisson(dims):
    """The Dirichlet 5-/7-point Poisson matrix of a dims grid, first index fastest (kron sums of tridiag(-1, 2, -1))."""
    import scipy.sparse as sp
    A = None
    for d in dims:
        T = sp.diags([-np.ones(d - 1), 2.0 * np.ones(d), -np.ones(d - 1)], [-1, 0, 1], format="csr")
        A = T if A is None else sp.kron(sp.identity(T.shape[0]), A) + sp.kron(T, sp.identity(A.shape[0]))
    A = sp.csr_matrix(A)
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


def low_eigenvectors(A, k, apply_jacobi):
    """The k lowest eigenvectors of M A (M = I or Jacobi) from a dense eigh of D^-1/2 A D^-1/2, and all its eigenvalues."""
    d = A.diagonal() if apply_jacobi else np.ones(A.shape[0])
    s = 1.0 / np.sqrt(d)
    lam, V = np.linalg.eigh(s[:, None] * A.toarray() * s[None, :])
    return s[:, None] * V[:, :k], lam
