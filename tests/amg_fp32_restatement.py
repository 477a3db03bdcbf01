"""The fp32 cycle of dpcg_set_precond_amg_precision (DPCG_AMG_FP32, include/dpcg.h) restated in numpy, on top of
tests/amg_restatement.py (the hierarchy, fp64 and unchanged) and tests/amg_smoother_restatement.py (the Chebyshev coefficients).

Everything is float64 except the stores the contract names, each an `astype(np.float32)` (round to nearest even):

  copies     the values of A_l, P_l (and so of P_l^T) and dinv_l of every level but the coarsest, rounded once;
  vectors    whatever the fp64 cycle stores to a work vector (x, r, Chebyshev's d, b of the levels >= 1, the coarse solution) is
             rounded where it is computed -- so r = b - A x is formed from the x that is stored;
  level 0    its right-hand side (PCG's r) is read unrounded and the result of its last smoothing step (z) is not rounded;
  coarsest   the dense inverse is float64; its input is the rounded b of that level and its output is rounded;
  Chebyshev  a step rounds d' = c1 d + c2 (dinv r), then x' = x + d', then r' = b - A x'; the last step of a level stores no d',
             so its d' is not rounded (x' is, except on level 0).
Jacobi (the default) and Chebyshev (pass the smoothers of amg_smoother_restatement.smoothers_for) are covered; Gauss-Seidel has
no fp32 cycle.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import amg_restatement as R
import amg_smoother_restatement as SR


def f32(v):
    """v rounded to fp32 and widened again."""
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


class Level32:
    """The fp32 copies of one smoothed level, widened to float64 for the arithmetic."""

    def __init__(self, lev: R.Level):
        self.A = sp.csr_matrix((f32(lev.A.data), lev.A.indices, lev.A.indptr), shape=lev.A.shape)
        P = sp.csr_matrix(lev.P)
        self.P = sp.csr_matrix((f32(P.data), P.indices, P.indptr), shape=P.shape)
        self.Pt = self.P.T.tocsr()
        self.dinv = f32(lev.dinv)


def copies(H: R.Hierarchy) -> list:
    return [Level32(lev) for lev in H.levels[:-1]]


def _jacobi(C: Level32, w: float, b, sweeps: int, top: bool, xc_of):
    d = C.dinv
    x = f32(w * d * b)
    r = f32(b - C.A @ x)
    for _ in range(sweeps - 1):
        x = f32(x + w * d * r)
        r = f32(b - C.A @ x)
    x = f32(x + C.P @ xc_of(f32(C.Pt @ r)))
    for k in range(sweeps):
        x = x + w * d * (b - C.A @ x)
        if not (top and k == sweeps - 1):
            x = f32(x)
    return x


def _chebyshev(C: Level32, sm: SR.Smoother, b, sweeps: int, top: bool, xc_of):
    dinv, deg = C.dinv, len(sm.c1)
    x, r, d = np.zeros_like(b), b, None                # pre-smoothing: from x = 0, r = b (level 0: unrounded)
    for t in range(sweeps * deg):
        k = t % deg
        d = f32(sm.c2[k] * (dinv * r) if k == 0 else sm.c1[k] * d + sm.c2[k] * (dinv * r))
        x = f32(x + d)
        r = f32(b - C.A @ x)
    x = f32(x + C.P @ xc_of(f32(C.Pt @ r)))
    r = f32(b - C.A @ x)
    for t in range(sweeps * deg):
        k = t % deg
        d = sm.c2[k] * (dinv * r) if k == 0 else sm.c1[k] * d + sm.c2[k] * (dinv * r)
        if t == sweeps * deg - 1:                      # the last step stores x' only
            x = x + d
            return x if top else f32(x)
        d = f32(d)
        x = f32(x + d)
        r = f32(b - C.A @ x)
    return x


def vcycle32(H: R.Hierarchy, b: np.ndarray, smoothers: list | None = None, sweeps: int | None = None, l: int = 0,
             _copies: list | None = None) -> np.ndarray:
    """One V(sweeps, sweeps) fp32 cycle from x = 0.  smoothers: None (damped Jacobi, sweeps = H.sweeps unless given) or the list
    of amg_smoother_restatement.smoothers_for (Jacobi and Chebyshev levels)."""
    C = copies(H) if _copies is None else _copies
    nu = H.sweeps if sweeps is None else sweeps
    b = np.asarray(b, dtype=np.float64)
    if l == len(H.levels) - 1:
        return f32(H.coarse_inv @ b) if l > 0 else H.coarse_inv @ b      # (one level: the dense inverse alone, fp64)
    xc_of = lambda bc: vcycle32(H, bc, smoothers, nu, l + 1, C)          # noqa: E731
    sm = smoothers[l] if smoothers is not None else None
    if sm is not None and sm.kind == SR.CHEBYSHEV:
        return _chebyshev(C[l], sm, b, nu, l == 0, xc_of)
    if sm is not None and sm.kind != SR.JACOBI:
        raise ValueError("the fp32 cycle smooths with Jacobi or Chebyshev")
    return _jacobi(C[l], H.levels[l].omega, b, nu, l == 0, xc_of)


class VCycle32:
    """`M @ r` by one fp32 cycle (what oracle.preconditioned_conjugate_gradient takes)."""

    def __init__(self, H: R.Hierarchy, smoothers: list | None = None, sweeps: int | None = None):
        self.H, self.smoothers, self.sweeps = H, smoothers, sweeps
        self._copies = copies(H)

    def __matmul__(self, r):
        return vcycle32(self.H, np.asarray(r, dtype=np.float64), self.smoothers, self.sweeps, 0, self._copies)
