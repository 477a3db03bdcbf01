"""The systems and expected values of the BiCGStab edge tests (test_bicgstab_edges_host.py on the CPU, test_bicgstab_edges_gpu.py and its
child process bicgstab_edges_child.py on the device).  numpy / scipy only.

What the 52 device tests of test_bicgstab_gpu.py never run, and which system here runs it:
  second and later trips of the 16-byte vector passes (n > 524 288, or a grid held small by DPCG_VEC_GRID in a child process)
                                  725x725_pe3 (n = 525 625, odd: 668 lanes take a second trip), 23x23_pe2 on ONE workgroup (264 pairs on
                                  256 lanes), 161x161_pe3 on three (12 960 pairs on 768 lanes: 17 trips, the last ragged)
  more than 256 partials          257x257_pe3 (G = 259: reduce_slots takes a second trip), 725x725_pe3 (G = 1024: all four; the SpMV's
                                  grid is above 1024 under the tile plan it takes by default and 2048 -- all eight slots of
                                  EarlyPartials -- with the CSR-stream kernel forced)
  A's tile and vector SpMV with a second vector in the dot epilogue
                                  forced by DPCG_SPMV_KERNEL on 64x64_pe5, 20x20x20_pe3, 12x12x12_pe3; by default on 725x725_pe3
                                  (tile), 13pt_24x24_pe20 and ragged_2001 (vector), mix_700 (tile with blocks that gather)
  the breakdown sites             BREAKDOWNS: small integers, every operation exact, so the device owes the restatement's bits

The short-run rule of test_bicgstab_gpu.py is used unchanged: max_iter = K updates, history[0..K] and x within 1e-10, 100 x a spread
between two CPU summation orders that test_bicgstab_edges_host.py asserts to be <= 1e-12 for every pair of SHORT_PAIRS at K_OF[pair].
K = 6 (bicgstab_cases.K) holds on every pair but one: 13pt_24x24_pe20 under the CSR M, where the Neumann-series M of A @ A at cell
Peclet number 20 is no approximate inverse and the residual GROWS (history 1, 7.05, 7.05, 29.9, 2398, ...): the spread is 2.1e-15 /
1.5e-14 / 2.3e-9 after 1 / 2 / 3 updates, so that pair runs 2 updates.  ragged_2001 under the CSR M converges inside the short run, after
5 updates, under both summation orders with stopping margins 6.5 and 6.4 (asserted on the CPU: >= bicgstab_cases.MARGIN).

M on the CPU is bicgstab_cases.precond_apply for the systems that module knows; for the systems made here `precond_apply` below builds
the same three M (identity, 1 / diagonal, bicgstab_cases.neumann_series_csr) from the matrix.
"""

import functools
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import bicgstab_cases as C
import bicgstab_restatement as R
from deeppreconditioning_amd.poisson import convection_diffusion_csr

K = C.K
RTOL_SQ = C.RTOL_SQ
SEED = C.SEED

# upwind convection-diffusion beyond bicgstab_cases.SYSTEMS: name -> (shape, peclet)
STENCILS = {
    "257x257_pe3": ((257, 257), 3.0),      # n = 66 049, odd: G = 259 vector workgroups
    "725x725_pe3": ((725, 725), 3.0),      # n = 525 625, odd: G = 1024, a second vector trip, the tile plan by default
    "20x20x20_pe3": ((20, 20, 20), 3.0),   # 7-point: tiles when forced
    "24x24_pe5": ((24, 24), 5.0),          # the pattern of 24x24_pe20 with other values (update_values)
}
VEC_GRID = {"257x257_pe3": 259, "725x725_pe3": 1024}
MIX_SIDE = 700


def _dominant(off):
    """off-diagonal part -> off + diag(row sums of |.| + 0.05), sorted CSR with int32 indices"""
    A = (off + sp.diags(np.asarray(abs(off).sum(axis=1)).ravel() + 0.05)).tocsr()
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


def thirteen_point():
    """(A @ A) of 24x24_pe20: 13 entries in an interior row, values not symmetric -- the vector kernel at 8 lanes a row by default"""
    A = C.matrix("24x24_pe20")
    B = (A @ A).tocsr()
    B.sort_indices()
    B.indices, B.indptr = B.indices.astype(np.int32), B.indptr.astype(np.int32)
    return B


def ragged(n=2001, seed=11):
    """row i holds 1 + (7 i mod 40) entries: a diagonal-only row next to rows of 40; off-diagonal values uniform in (-1, 1), not
    mirrored (the pattern is not symmetric either); strictly row dominant"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        k = (7 * i) % 40
        c = rng.choice(n - 1, size=k, replace=False)
        c = c + (c >= i)                                   # skips the diagonal
        rows.append(np.full(k, i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    off = sp.coo_matrix((rng.uniform(-1.0, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    return _dominant(off)


def mixed_tiles():
    """The system of test_spmv_tile_plan_with_blocks_that_gather (5-point Poisson on 700 x 700; every ninth 256-row block gets 60
    couplings to far places, mirrored), its strict upper triangle multiplied by 0.9 -- values no longer symmetric -- and the diagonal
    raised to the rows' sums of |.| where the row is short of it (no row is: scaling only lowers the sums; kept as the construction)."""
    from oracle import oracle as O
    m = MIX_SIDE
    A0 = O.poisson2d(m)
    n = A0.shape[0]
    rng = np.random.default_rng(3)
    blocks = np.arange(0, n // 256, 9)
    rows = (blocks[:, None] * 256 + rng.integers(0, 256, (blocks.size, 60))).ravel()
    cols = rng.integers(0, n, rows.size)
    keep = np.abs(rows - cols) > 4 * m
    E = sp.coo_matrix((np.full(int(keep.sum()), -0.25), (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    E.sum_duplicates()
    Esym = (E + E.T).tocsr()
    S = (A0 + Esym + sp.diags(np.asarray(abs(Esym).sum(axis=1)).ravel())).tocsr()
    A = (sp.tril(S, 0) + 0.9 * sp.triu(S, 1)).tocsr()
    off = A - sp.diags(A.diagonal())
    short = np.maximum(np.asarray(abs(off).sum(axis=1)).ravel() - A.diagonal(), 0.0)
    A = (A + sp.diags(short)).tocsr()
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


BUILT = {"13pt_24x24_pe20": thirteen_point, "ragged_2001": ragged, "mix_700": mixed_tiles}


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name in C.SYSTEMS:
        return C.matrix(name)
    if name in STENCILS:
        return convection_diffusion_csr(*STENCILS[name])
    return BUILT[name]()


def rhs(name, seed=SEED):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, matrix(name).shape[0])


def x0_of(name):
    """the nonzero start of the child process' x0 runs"""
    return np.random.default_rng(5).uniform(-1.0, 1.0, matrix(name).shape[0])


def precond_apply(name, pre):
    """the CPU M of a tag: bicgstab_cases.precond_apply where that module knows the system, the same three M otherwise"""
    if name in C.SYSTEMS:
        return C.precond_apply(name, pre)
    A = matrix(name)
    if pre == "none":
        return None
    if pre == "jacobi":
        dinv = 1.0 / A.diagonal()
        return lambda v: dinv * v
    if pre == "csr":
        M = C.neumann_series_csr(A)
        return lambda v: M @ v
    raise KeyError(pre)


@functools.lru_cache(maxsize=None)
def restated(name, pre, max_iter=K, strided=False, x0=False):
    return R.bicgstab(matrix(name), rhs(name), precond_apply(name, pre), x0=x0_of(name) if x0 else None, rtol_sq=RTOL_SQ,
                      max_iter=max_iter, dot=R.strided_dot if strided else R.plain_dot)


def short_spread(name, pre, k, x0=False):
    """(history spread, x spread) of the restatement between the two summation orders after k updates"""
    a, c = restated(name, pre, k, False, x0), restated(name, pre, k, True, x0)
    if len(a["history"]) != len(c["history"]):
        return np.inf, np.inf
    return R.rel_spread(a["history"], c["history"]), R.x_spread(a["x"], c["x"])


# ---- A. trips and partial counts --------------------------------------------------------------------------------------------------
# the child process: DPCG_VEC_GRID -> (system, pairs of 16 bytes, lanes, trips of the busiest lane)
CHILD = {1: ("23x23_pe2", 264, 256, 2), 3: ("161x161_pe3", 12960, 768, 17)}
CHILD_X0_PRE = "jacobi"                    # the preconditioner of the one run from a nonzero x0
NATURAL = [("257x257_pe3", "none"), ("257x257_pe3", "jacobi"), ("257x257_pe3", "csr"), ("725x725_pe3", "none"), ("725x725_pe3", "jacobi")]

# ---- B. every SpMV plan ---------------------------------------------------------------------------------------------------------------
FORCED = [("tile", "64x64_pe5"), ("tile", "20x20x20_pe3"), ("vector", "64x64_pe5"), ("vector", "12x12x12_pe3"),
          ("stream", "64x64_pe5"), ("stream", "20x20x20_pe3")]
VECTOR_BY_DEFAULT = {"13pt_24x24_pe20": 8, "ragged_2001": 16}      # -> lanes a row (make_plan: doubled while twice it < nnz / n)
MIX = "mix_700"

# ---- C. the handle's life ---------------------------------------------------------------------------------------------------------------
LIFE_SYSTEM = "24x24_pe20"
LIFE_ORDER = ["none", "jacobi", "csr", "ilut_solve", "none"]      # ilut_solve: ILUT("solve", threshold=1e-3) in bicgstab_cases
NEW_VALUES = "24x24_pe5"
LIFE_PAIRS = [(NEW_VALUES, "jacobi"), (NEW_VALUES, "csr")]      # (the pairs of LIFE_SYSTEM are bicgstab_cases' own)

SHORT_PAIRS = sorted({(n, p) for _, n in FORCED for p in C.PRECONDS} | {(n, p) for n in VECTOR_BY_DEFAULT for p in C.PRECONDS} |
                     {(MIX, p) for p in C.PRECONDS} | set(NATURAL) | set(LIFE_PAIRS))
K_OF = {pair: K for pair in SHORT_PAIRS}
K_OF[("13pt_24x24_pe20", "csr")] = 2        # the spread is 2.3e-9 after 3 updates: see the head of this file
STOPS_INSIDE = {("ragged_2001", "csr"): 5}  # pairs whose short run ends by convergence, and after how many updates

# ---- D. the breakdown sites ---------------------------------------------------------------------------------------------------------------
# name -> (A, b, statement that breaks, status, updates, history, x).  M = I, no reordering.  All entries small integers: every
# product, sum and quotient of the recurrence is a dyadic rational that fp64 holds, so no summation order can change a bit.
BREAKDOWNS = {
    # update 0: p = r = (1,0), v = A p = (0,-1) != 0, <rhat,v> = 0
    "pass_s_rhat_v": (np.array([[0.0, 1.0], [-1.0, 0.0]]), np.array([1.0, 0.0]), "rv", R.BREAKDOWN, 0, [1.0], [0.0, 0.0]),
    # update 0: v = (2,0), alpha = 1, s = (-1,1) != 0, t = A s = 0: <t,t> = 0.  x must not have taken alpha ph.
    "pass_x_t_t": (np.array([[1.0, 1.0], [0.0, 0.0]]), np.array([1.0, 1.0]), "tt", R.BREAKDOWN, 0, [1.0], [0.0, 0.0]),
    # update 0 completes with alpha = -1/2, omega = 0 (<t,s> = 0), r = s = (0,-1); update 1: <rhat,r> = 0
    "pass_p_rho_omega_0": (np.array([[-2.0, -2.0], [-2.0, 0.0]]), np.array([1.0, 0.0]), "rho", R.BREAKDOWN, 1, [1.0, 1.0], [-0.5, 0.0]),
    # update 0 completes with alpha = 1/2, omega = 1/2, x = (1/2,-1/4,1/4), r = (0,0,1/2); update 1: <rhat,r> = 0.  Three rows: on two,
    # <rhat,r> = 0 after a completed update forces omega = 0 (s is orthogonal to rhat, so A s must be too: s is an eigenvector and
    # r = 0).  With omega = 0 (the case above) a pass P that missed the test computes beta = 0 x inf, a NaN that pass S reports as the
    # same BREAKDOWN at the same count; with omega != 0 it goes on with beta = 0 -- a restart from r -- and completes update 1.
    "pass_p_rho": (np.array([[2.0, 2.0, 2.0], [1.0, 1.0, -1.0], [-1.0, 0.0, 0.0]]), np.array([1.0, 0.0, 0.0]), "rho", R.BREAKDOWN, 1,
                   [1.0, 0.25], [0.5, -0.25, 0.25]),
}
KRON = 513                                  # kron(I_513, A): n = 1026 (1539 for the three-row case) -- five (seven) workgroups that must all decide alike


def breakdown_system(name, copies=1):
    """-> (rowptr, col, val, b) of kron(I_copies, A) with every entry of A stored (zeros too: no row is empty, the pattern is dense
    m x m blocks), b tiled"""
    A, b = BREAKDOWNS[name][:2]
    m = b.size
    rowptr = m * np.arange(m * copies + 1, dtype=np.int32)
    col = (m * np.repeat(np.arange(copies, dtype=np.int32), m * m) + np.tile(np.arange(m, dtype=np.int32), m * copies)).astype(np.int32)
    return rowptr, col, np.tile(A.ravel(), copies), np.tile(b, copies)


def breakdown_csr(name, copies=1):
    rowptr, col, val, b = breakdown_system(name, copies)
    return sp.csr_matrix((val, col, rowptr), shape=(b.size, b.size)), b


def exact_scalars(A, b, updates):
    """The scalars of the recurrence in rational arithmetic (M = I, x0 = 0), update by update until one of them is 0:
    -> list of dicts with rho, rv, alpha, ts, tt, omega (Fractions; a key is absent from the statement that breaks on)."""
    F = lambda v: [Fraction(float(e)) for e in v]                    # noqa: E731
    Am = [F(row) for row in A]
    mv = lambda v: [sum(a * e for a, e in zip(row, v)) for row in Am]    # noqa: E731
    dot = lambda u, v: sum(a * e for a, e in zip(u, v))                  # noqa: E731
    r = F(b)
    rhat, p, v = list(r), [Fraction(0)] * len(r), [Fraction(0)] * len(r)
    rho = alpha = omega = Fraction(1)
    out = []
    for _ in range(updates + 1):
        rec = {"rho": dot(rhat, r)}
        out.append(rec)
        if rec["rho"] == 0:
            break
        beta = (rec["rho"] / rho) * (alpha / omega)
        rho = rec["rho"]
        p = [ri + beta * (pi - omega * vi) for ri, pi, vi in zip(r, p, v)]
        v = mv(p)
        rec["rv"] = dot(rhat, v)
        rec["v_nonzero"] = any(v)
        if rec["rv"] == 0:
            break
        alpha = rec["alpha"] = rho / rec["rv"]
        s = [ri - alpha * vi for ri, vi in zip(r, v)]
        rec["s_nonzero"] = any(s)
        t = mv(s)
        rec["ts"], rec["tt"] = dot(s, t), dot(t, t)
        if rec["tt"] == 0:
            break
        omega = rec["omega"] = rec["ts"] / rec["tt"]
        r = [si - omega * ti for si, ti in zip(s, t)]
    return out


# the half-step exit with five workgroups and the odd tail: a diagonal system under Jacobi (s = r - 1 x r up to rounding)
HALF_N = 1025
HALF_BOUND = 16 * 2.0 ** -106              # derived in test_bicgstab_gpu.py::test_half_step_exit_and_cap


def half_step_system():
    d = np.linspace(1.0, 3.0, HALF_N)
    return sp.diags(d).tocsr(), d, np.arange(1.0, HALF_N + 1.0)
