"""The factorised sparse approximate inverse (FSAI; Kolotilina & Yeremin, SIAM J. Matrix Anal. Appl. 14 (1993)) restated in
numpy -- the contract of the device routine behind dpcg_set_precond_fsai / dpcg_set_precond_fsai_pattern
(deeppreconditioning_amd/csrc/dpcg_fsai.hip).

P is a symmetric pattern that contains the diagonal; for column i, P_i = { j >= i : (j, i) in P } in ascending order (its first
element is i) and m_i = |P_i|.  With B = A[P_i, P_i] (dense, m_i x m_i):

    B y = e_1,        L[P_i, i] = y / sqrt(y_1)

so that M = L L^T approximates A^-1.  Everything happens in the caller's numbering.

THE ORDER OF OPERATIONS (the device follows it; -ffp-contract=off, one product and one subtraction at a time, fp64 sqrt and /
correctly rounded -- so the two agree bit for bit).  Only the lower triangle of B is read: b_pq = A[P_i[p], P_i[q]] for q <= p, an
entry absent from A's pattern is 0.0.

  1. Cholesky B = C C^T, column by column j = 0 .. m-1, every sum over ascending k:
         s = b_pj;  for k = 0 .. j-1: s = s - c_pk * c_jk          (p = j .. m-1)
         c_jj = sqrt(s_j)   (s_j must be finite and > 0: else the pivot error names column i);   c_pj = s_p / c_jj  (p > j)
  2. forward substitution C w = e_1, column-oriented: s_0 = 1.0, s_p = 0.0 (p > 0); for j = 0 .. m-1:
         w_j = s_j / c_jj;  s_p = s_p - c_pj * w_j  (p > j)        (per entry: k ascending)
  3. backward substitution C^T y = w, column-oriented: s = w; for j = m-1 .. 0:
         y_j = s_j / c_jj;  s_p = s_p - c_jp * y_j  (p < j)        (per entry: k descending)
  4. l_p = y_p / sqrt(y_0)   (y_0 must be finite and > 0: pivot error)

There is no tree-shaped sum in any width class of the device kernels: every entry's sum is sequential in the order above.

`level = k` (1, 2 or 3): P = the pattern of A^k as a structural power (no numerical cancellation; stored zeros of A count).
`pattern`: a lower-triangular CSR pattern (values ignored) with the diagonal in every row and ascending columns = tril(P) by rows.
"""

import numpy as np
import scipy.sparse as sp

MAX_M = 64          # the device's limit on m_i
WIDTH_CLASSES = (4, 8, 16, 32, 64)


class FsaiError(ValueError):
    def __init__(self, kind, column, message):
        super().__init__(message)
        self.kind, self.column = kind, column


def _pattern_csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return sp.csr_matrix((np.ones(A.indices.size, dtype=np.int64), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def power_pattern(A, level):
    """The structural pattern of A^level as sorted CSR (data all ones)."""
    if level not in (1, 2, 3):
        raise FsaiError("level", -1, "fsai: level must be 1, 2 or 3")
    S = _pattern_csr(A)
    P = S
    for _ in range(level - 1):
        P = P @ S                                     # (positive counts: no cancellation)
        P.data[:] = 1
        P.sort_indices()
    return P


def upper_pattern(A=None, level=None, pattern=None):
    """(indptr, indices) of the sets P_i: row i lists P_i ascending (the upper triangle of P by rows)."""
    if (level is None) == (pattern is None):
        raise FsaiError("arguments", -1, "fsai: give either level or pattern")
    if pattern is not None:
        Lp = sp.csr_matrix(pattern)
        if not Lp.has_sorted_indices:
            raise FsaiError("pattern", -1, "fsai: the pattern must have ascending columns")
        n = Lp.shape[0]
        rows = np.repeat(np.arange(n), np.diff(Lp.indptr))
        if np.any(Lp.indices > rows):
            raise FsaiError("pattern", -1, "fsai: the pattern must be lower triangular")
        last = Lp.indptr[1:] - 1
        if np.any(np.diff(Lp.indptr) == 0) or np.any(Lp.indices[last] != np.arange(n)):
            raise FsaiError("diagonal", -1, "fsai: the pattern must contain the diagonal")
        U = sp.csr_matrix((np.ones(Lp.indices.size, dtype=np.int64), Lp.indices, Lp.indptr), shape=Lp.shape).T.tocsr()
    else:
        U = sp.triu(power_pattern(A, level), format="csr")
    U.sort_indices()
    n = U.shape[0]
    first = U.indptr[:-1]
    if np.any(np.diff(U.indptr) == 0) or np.any(U.indices[first] != np.arange(n)):
        bad = int(np.flatnonzero((np.diff(U.indptr) == 0) | (U.indices[np.minimum(first, U.indices.size - 1)] != np.arange(n)))[0])
        raise FsaiError("diagonal", bad, f"fsai: structurally missing diagonal at column {bad}")
    return U.indptr.astype(np.int64), U.indices.astype(np.int64)


def local_systems(A, cols, up, ui, m):
    """The dense lower triangles B[c, p, q] = A[P_i[p], P_i[q]] (q <= p, 0.0 elsewhere and where A has no entry) of the columns
    `cols`, all with m_i = m: plain index arithmetic on keys row * n + col of A's sorted CSR."""
    n = A.shape[0]
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    P = ui[up[cols][:, None] + np.arange(m)[None, :]]                # (c, m)
    want = P[:, :, None] * n + P[:, None, :]                         # (c, p, q): row P[p], column P[q]
    pos = np.searchsorted(keys, want)
    pos_c = np.minimum(pos, keys.size - 1)
    hit = keys[pos_c] == want
    B = np.where(hit, A.data[pos_c], 0.0)
    return np.tril(B), P


def solve_columns(B):
    """Steps 1-4 for a batch B[c, m, m] (lower triangles).  Returns (l[c, m], bad[c]): bad marks a failed pivot."""
    c, m = B.shape[0], B.shape[1]
    C = np.zeros_like(B)
    bad = np.zeros(c, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(m):
            s = B[:, j:, j].copy()
            for k in range(j):
                s = s - C[:, j:, k] * C[:, j, k][:, None]
            bad |= ~(np.isfinite(s[:, 0]) & (s[:, 0] > 0.0))
            d = np.sqrt(s[:, 0])
            C[:, j, j] = d
            C[:, j + 1:, j] = s[:, 1:] / d[:, None]
        s = np.zeros((c, m))
        s[:, 0] = 1.0
        w = np.zeros((c, m))
        for j in range(m):
            w[:, j] = s[:, j] / C[:, j, j]
            s[:, j + 1:] = s[:, j + 1:] - C[:, j + 1:, j] * w[:, j][:, None]
        s = w.copy()
        y = np.zeros((c, m))
        for j in range(m - 1, -1, -1):
            y[:, j] = s[:, j] / C[:, j, j]
            s[:, :j] = s[:, :j] - C[:, j, :j] * y[:, j][:, None]
        bad |= ~(np.isfinite(y[:, 0]) & (y[:, 0] > 0.0))
        l = y / np.sqrt(y[:, 0])[:, None]
    return l, bad


def fsai_upper(A, level=None, pattern=None, max_m=MAX_M):
    """H = L^T by rows: (indptr, indices, values) -- row i holds P_i and the solve of column i."""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    if level is not None and pattern is None:
        n = A.shape[0]
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        has_diag = np.zeros(n, dtype=bool)
        has_diag[rows[A.indices == rows]] = True
        if not has_diag.all():
            bad = int(np.flatnonzero(~has_diag)[0])
            raise FsaiError("diagonal", bad, f"fsai: structurally missing diagonal at column {bad}")
    up, ui = upper_pattern(A, level, pattern)
    mi = np.diff(up)
    if mi.max() > max_m:
        bad = int(np.flatnonzero(mi > max_m)[0])
        raise FsaiError("width", bad, f"fsai: column {bad} has m = {int(mi[bad])} > {max_m}")
    hv = np.zeros(ui.size)
    failed = []
    for m in np.unique(mi):
        cols = np.flatnonzero(mi == m)
        for c0 in range(0, cols.size, 1 << 15):
            cc = cols[c0:c0 + (1 << 15)]
            B, _ = local_systems(A, cc, up, ui, int(m))
            l, bad = solve_columns(B)
            hv[up[cc][:, None] + np.arange(m)[None, :]] = l
            failed.extend(cc[bad].tolist())
    if failed:
        col = min(failed)
        raise FsaiError("pivot", col, f"fsai: non-positive or non-finite pivot in the local system of column {col}")
    return up, ui, hv


def fsai(A, level=None, pattern=None, max_m=MAX_M):
    """L (scipy CSR, lower triangular, columns ascending, the diagonal last in every row) with M = L L^T ~ A^-1."""
    up, ui, hv = fsai_upper(A, level, pattern, max_m)
    n = up.size - 1
    # the transpose of H by a stable sort of its entries by column: rows of L ascend in the column index
    order = np.argsort(ui, kind="stable")
    rows_of = np.repeat(np.arange(n), np.diff(up))
    lp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(ui, minlength=n), out=lp[1:])
    L = sp.csr_matrix((hv[order], rows_of[order].astype(np.int32), lp), shape=(n, n))
    return L


def width_class_counts(A, level=None, pattern=None):
    """Columns per width class (m <= 4, 8, 16, 32, 64) and max m -- what dpcg_get_fsai_info reports."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    up, _ = upper_pattern(A, level, pattern)
    mi = np.diff(up)
    counts, lo = [], 0
    for w in WIDTH_CLASSES:
        counts.append(int(np.count_nonzero((mi > lo) & (mi <= w))))
        lo = w
    return counts, int(mi.max())
