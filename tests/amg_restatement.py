"""Smoothed-aggregation multigrid restated in numpy / scipy: the contract of dpcg_set_precond_amg (include/dpcg.h).

Every rule that looks at a row index uses the index of the matrix handed in (the caller's numbering), so the aggregates are
integers the device must reproduce exactly; P, the Galerkin operators and the V-cycle agree to rounding (their sums run in
another order here).  omega is either given per level (the library's, from its Lanczos estimate) or computed here from the exact
lambda_max(D^-1 A) (the CPU tests).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

OUT, UND, IN = 0, 1, 2


def splitmix(seed: int, idx: np.ndarray) -> np.ndarray:
    """h(seed, i): the splitmix64 finaliser of the counter seed * phi + (i + 1) * c (k_lz_start / k_mis_init), as uint64."""
    with np.errstate(over="ignore"):
        x = (np.uint64(seed & (2**64 - 1)) * np.uint64(0x9E3779B97F4A7C15)
             + (np.asarray(idx, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def strength(A: sp.csr_matrix, theta: float = 0.0) -> sp.csr_matrix:
    """Strong connections (data = |a_ij|): j != i, a_ij != 0 and |a_ij| >= theta sqrt(|a_ii a_jj|)."""
    C = A.tocoo()
    d = A.diagonal()
    keep = (C.row != C.col) & (C.data != 0) & (np.abs(C.data) >= theta * np.sqrt(np.abs(d[C.row] * d[C.col])))
    S = sp.csr_matrix((np.abs(C.data[keep]), (C.row[keep], C.col[keep])), shape=A.shape)
    S.sort_indices()
    return S


def _closed_max(S: sp.csr_matrix, v: np.ndarray) -> np.ndarray:
    """max(v[i], max_{j strong neighbour of i} v[j])."""
    out = v.copy()
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    np.maximum.at(out, rows, v[S.indices])
    return out


def mis2(S: sp.csr_matrix, seed: int = 0) -> np.ndarray:
    """Roots (bool) of the deterministic parallel MIS(2) on tuples (state, h(seed, i), i)."""
    n = S.shape[0]
    idx = np.arange(n)
    h = splitmix(seed, idx)
    state = np.full(n, UND, dtype=np.int64)
    for _ in range(100000):
        order = np.lexsort((idx, h, state))          # ascending tuples
        rank = np.empty(n, dtype=np.int64)
        rank[order] = idx
        m2 = _closed_max(S, _closed_max(S, rank))
        win = order[m2]
        und = state == UND
        new = state.copy()
        new[und & (win == idx)] = IN
        new[und & (win != idx) & (state[win] == IN)] = OUT
        state = new
        if not (state == UND).any():
            return state == IN
    raise RuntimeError("MIS(2) did not terminate")


def aggregate(A: sp.csr_matrix, S: sp.csr_matrix, roots: np.ndarray) -> np.ndarray:
    """Aggregate of every row: roots numbered by ascending index; a root's strong neighbours join it; the rest join their
    step-1-assigned strong neighbour of largest |a_ij| (ties: the smaller index)."""
    n = A.shape[0]
    agg = np.full(n, -1, dtype=np.int64)
    agg[roots] = np.arange(int(roots.sum()))
    C = S.tocoo()
    near = roots[C.col] & ~roots[C.row]
    agg[C.row[near]] = agg[C.col[near]]
    rest = agg < 0
    cand = rest[C.row] & (agg[C.col] >= 0)
    r, c = C.row[cand], C.col[cand]
    w = C.data[cand]                                  # |a_ij|
    order = np.lexsort((c, -w, r))
    r, c = r[order], c[order]
    first = np.r_[True, r[1:] != r[:-1]] if r.size else np.zeros(0, dtype=bool)
    final = agg.copy()
    final[r[first]] = agg[c[first]]
    if (final < 0).any():
        raise RuntimeError("a row without an aggregate")
    return final.astype(np.int32)


def tentative(agg: np.ndarray) -> sp.csr_matrix:
    n, nc = agg.size, int(agg.max()) + 1
    size = np.bincount(agg, minlength=nc)
    return sp.csr_matrix((1.0 / np.sqrt(size[agg].astype(np.float64)), agg, np.arange(n + 1)), shape=(n, nc))


def lambda_max_dinv_a(A: sp.csr_matrix) -> float:
    """lambda_max(D^-1 A) of an SPD A (that of the symmetric D^-1/2 A D^-1/2)."""
    d = 1.0 / np.sqrt(A.diagonal())
    B = sp.diags(d) @ A @ sp.diags(d)
    if A.shape[0] <= 2000:
        return float(np.linalg.eigvalsh(B.toarray())[-1])
    from scipy.sparse.linalg import eigsh
    return float(eigsh(B, k=1, which="LA", tol=1e-10)[0][0])


@dataclass
class Level:
    A: sp.csr_matrix
    dinv: np.ndarray
    agg: np.ndarray | None = None
    P: sp.csr_matrix | None = None
    omega: float = 0.0


@dataclass
class Hierarchy:
    levels: list = field(default_factory=list)
    coarse_inv: np.ndarray | None = None
    sweeps: int = 1


def hierarchy(A: sp.csr_matrix, theta: float = 0.0, max_levels: int = 10, max_coarse: int = 500, seed: int = 0,
              omegas=None, sweeps: int = 1) -> Hierarchy:
    """The hierarchy dpcg_set_precond_amg builds; omegas[l] (optional): the smoothing weight of level l."""
    H = Hierarchy(sweeps=sweeps)
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    for l in range(max_levels):
        n = A.shape[0]
        lev = Level(A, 1.0 / A.diagonal())
        H.levels.append(lev)
        if n <= max_coarse or l == max_levels - 1:
            break
        S = strength(A, theta)
        roots = mis2(S, seed)
        nc = int(roots.sum())
        if nc == 0 or nc > 0.9 * n:
            break
        agg = aggregate(A, S, roots)
        T = tentative(agg)
        omega = omegas[l] if omegas is not None else (4.0 / 3.0) / lambda_max_dinv_a(A)
        P = (T - sp.diags(omega * lev.dinv) @ (A @ T)).tocsr()
        lev.agg, lev.P, lev.omega = agg, P, omega
        A = (P.T @ (A @ P)).tocsr()
        A.sort_indices()
    H.coarse_inv = np.linalg.inv(H.levels[-1].A.toarray())
    return H


def vcycle(H: Hierarchy, b: np.ndarray, l: int = 0) -> np.ndarray:
    """One V(nu, nu) cycle with damped Jacobi from x = 0 (the device's order of operations)."""
    lev = H.levels[l]
    if l == len(H.levels) - 1:
        return H.coarse_inv @ b
    A, w, d = lev.A, lev.omega, lev.dinv
    x = w * d * b
    r = b - A @ x
    for _ in range(H.sweeps - 1):
        x = x + w * d * r
        r = b - A @ x
    x = x + lev.P @ vcycle(H, lev.P.T @ r, l + 1)
    for _ in range(H.sweeps):
        x = x + w * d * (b - A @ x)
    return x


class VCycle:
    """`M @ r` by one V-cycle (what oracle.preconditioned_conjugate_gradient takes)."""

    def __init__(self, H: Hierarchy):
        self.H = H

    def __matmul__(self, r):
        return vcycle(self.H, np.asarray(r, dtype=np.float64))


def dense_operator(H: Hierarchy) -> np.ndarray:
    n = H.levels[0].A.shape[0]
    return np.column_stack([vcycle(H, e) for e in np.eye(n)])
