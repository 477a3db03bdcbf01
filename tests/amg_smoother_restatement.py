"""The smoothers of dpcg_set_precond_amg_smoothed restated in numpy / scipy, on top of tests/amg_restatement.py.

The hierarchy (A_l, P_l, omega_l) comes from amg_restatement (or from the device, level by level); the colourings, rho_l and
hence the Chebyshev coefficients are handed in, so that a test can replay exactly what the device built.  Vectors may be 1-D or
2-D (one column per right-hand side: the dense operator in one call).

  Gauss-Seidel   a pass over colour class K: x_K += dinv_K (b_K - A_K x) (all rows of K at once, the diagonal included);
                 a symmetric sweep: the classes 0, 1, .., m-1, m-2, .., 0.
  Chebyshev      u = rho, lo = u / eig_ratio, theta = (u + lo) / 2, delta = (u - lo) / 2, sigma = theta / delta;
                 r = b - A x, d = c2_0 (dinv r), x += d; then per step d = c1_k d + c2_k (dinv r), x += d, with
                 rho_0 = 1 / sigma, rho_1 = 1 / (2 sigma - rho_0), c1_k = rho_1 rho_0, c2_k = 2 rho_1 / delta (Saad, Jacobi-preconditioned).
  Jacobi         x += omega dinv (b - A x).
Each is applied `sweeps` times before the coarse correction (from x = 0) and after it.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import amg_restatement as R

JACOBI, GAUSS_SEIDEL, CHEBYSHEV = "jacobi", "gauss_seidel", "chebyshev"


def greedy_colors(A: sp.csr_matrix) -> np.ndarray:
    """A proper colouring of A's graph: rows in order, each the smallest colour none of its coloured neighbours has."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    color = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        nb = A.indices[A.indptr[i]:A.indptr[i + 1]]
        used = set(color[nb[nb != i]].tolist())
        c = 0
        while c in used:
            c += 1
        color[i] = c
    return color.astype(np.int32)


def color_classes(colors: np.ndarray) -> list:
    """The rows of each colour, ascending, colour by colour."""
    colors = np.asarray(colors)
    return [np.nonzero(colors == c)[0] for c in range(int(colors.max()) + 1)]


def is_proper(A: sp.csr_matrix, colors: np.ndarray) -> bool:
    C = sp.csr_matrix(A).tocoo()
    off = C.row != C.col
    return bool(np.all(colors[C.row[off]] != colors[C.col[off]]))


def _col(v: np.ndarray, like: np.ndarray) -> np.ndarray:
    return v[:, None] if like.ndim == 2 else v


def gs_pass(A, dinv, b, x, rows, A_rows=None):
    """One colour pass, in place (A_rows: A[rows], when the caller has it already)."""
    A_rows = A[rows] if A_rows is None else A_rows
    x[rows] = x[rows] + _col(dinv[rows], x) * (b[rows] - A_rows @ x)
    return x


def gs_sweep(A, dinv, b, x, classes, blocks=None):
    m = len(classes)
    for c in list(range(m)) + list(range(m - 2, -1, -1)):
        gs_pass(A, dinv, b, x, classes[c], None if blocks is None else blocks[c])
    return x


def chebyshev_coefficients(rho: float, degree: int, eig_ratio: float):
    """(c1, c2, lower, upper), computed in the order the library computes them (the same bits)."""
    u = float(rho)
    lo = u / eig_ratio
    theta, delta = (u + lo) / 2.0, (u - lo) / 2.0
    sigma = theta / delta
    c1, c2 = [0.0] * degree, [0.0] * degree
    c2[0] = 1.0 / theta
    rho0 = 1.0 / sigma
    for k in range(1, degree):
        rho1 = 1.0 / (2.0 * sigma - rho0)
        c1[k] = rho1 * rho0
        c2[k] = 2.0 * rho1 / delta
        rho0 = rho1
    return c1, c2, lo, u


def chebyshev(A, dinv, b, x, c1, c2):
    """One application of the Chebyshev smoother to (x, b); returns the new x."""
    r = b - A @ x
    d = None
    for k in range(len(c1)):
        dk = _col(dinv, r) * r
        d = c2[k] * dk if k == 0 else c1[k] * d + c2[k] * dk
        x = x + d
        r = b - A @ x
    return x


@dataclass
class Smoother:
    kind: str
    omega: float = 0.0
    classes: list | None = None
    blocks: list | None = None        # A[rows] of every class
    c1: list | None = None
    c2: list | None = None


def smoothers_for(H: R.Hierarchy, kind: str, *, degree: int = 2, eig_ratio: float = 30.0, rhos=None, colorings=None, kinds=None):
    """The smoother of every smoothed level.  rhos[l] (default: (4/3) / omega_l, the exact lambda_max of an R.hierarchy) feeds
    Chebyshev; colorings[l] (default: greedy_colors) feeds Gauss-Seidel; kinds[l] overrides `kind` per level (a fallback)."""
    out = []
    for l, lev in enumerate(H.levels[:-1]):
        k = kinds[l] if kinds is not None else kind
        if k == GAUSS_SEIDEL:
            col = colorings[l] if colorings is not None else greedy_colors(lev.A)
            classes = color_classes(col)
            out.append(Smoother(k, lev.omega, classes=classes, blocks=[lev.A[rows] for rows in classes]))
        elif k == CHEBYSHEV:
            rho = rhos[l] if rhos is not None else (4.0 / 3.0) / lev.omega
            c1, c2, _, _ = chebyshev_coefficients(rho, degree, eig_ratio)
            out.append(Smoother(k, lev.omega, c1=c1, c2=c2))
        else:
            out.append(Smoother(JACOBI, lev.omega))
    return out


def smooth(lev: R.Level, sm: Smoother, b, x, sweeps: int):
    """`sweeps` applications of the level's smoother to (x, b); x = None: from x = 0."""
    x = np.zeros_like(b) if x is None else x.copy()
    for _ in range(sweeps):
        if sm.kind == GAUSS_SEIDEL:
            gs_sweep(lev.A, lev.dinv, b, x, sm.classes, sm.blocks)
        elif sm.kind == CHEBYSHEV:
            x = chebyshev(lev.A, lev.dinv, b, x, sm.c1, sm.c2)
        else:
            x = x + sm.omega * _col(lev.dinv, b) * (b - lev.A @ x)
    return x


def vcycle(H: R.Hierarchy, smoothers: list, b: np.ndarray, sweeps: int = 1, l: int = 0) -> np.ndarray:
    """One V(sweeps, sweeps) cycle: pre-smooth from x = 0, restrict b - A x with P^T, correct with P, post-smooth."""
    lev = H.levels[l]
    if l == len(H.levels) - 1:
        return H.coarse_inv @ b
    x = smooth(lev, smoothers[l], b, None, sweeps)
    r = b - lev.A @ x
    x = x + lev.P @ vcycle(H, smoothers, lev.P.T @ r, sweeps, l + 1)
    return smooth(lev, smoothers[l], b, x, sweeps)


class VCycle:
    """`M @ r` by one cycle (what oracle.preconditioned_conjugate_gradient takes)."""

    def __init__(self, H: R.Hierarchy, smoothers: list, sweeps: int = 1):
        self.H, self.smoothers, self.sweeps = H, smoothers, sweeps

    def __matmul__(self, r):
        return vcycle(self.H, self.smoothers, np.asarray(r, dtype=np.float64), self.sweeps)


def dense_operator(H: R.Hierarchy, smoothers: list, sweeps: int = 1) -> np.ndarray:
    n = H.levels[0].A.shape[0]
    return vcycle(H, smoothers, np.eye(n), sweeps)
