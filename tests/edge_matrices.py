"""Small SPD test matrices at the edges of the device AMG and ILUT setups: fp64 CSR, sorted indices, symmetric.

Every generator is deterministic (its seed is an argument).  Explicit zeros are kept where a generator stores them on purpose
(`with_stored_zeros`); the others hold no stored zeros.  `product_counts` is the per-row work of a row-wise SpGEMM X Y: the
number of products row i expands, sum over k in row i of X of nnz(Y[k, :]) -- what k_spgemm compares with its LDS capacity.
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def csr(A) -> sp.csr_matrix:
    """fp64 CSR with sorted indices and duplicates summed; stored zeros are kept."""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A


def _tri(m: int) -> sp.csr_matrix:
    return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1], format="csr")


def anisotropic2d(m: int, eps: float) -> sp.csr_matrix:
    """eps d_xx + d_yy on an m x m grid (Dirichlet): x couplings -eps, y couplings -1; row iy * m + ix."""
    I = sp.identity(m, format="csr")
    return csr(eps * sp.kron(I, _tri(m)) + sp.kron(_tri(m), I))


def _block_checkerboard(shape, block: int, contrast: float) -> np.ndarray:
    idx = np.indices(shape).sum(axis=0) if block <= 0 else sum(np.indices(shape)[d] // block for d in range(len(shape)))
    return np.where(idx % 2 == 0, 1.0, contrast)


def jumping(shape, block: int, contrast: float = 1e6) -> sp.csr_matrix:
    """-div(k grad u) by cell-centred finite volumes on a grid of `shape` (2-D or 3-D) cells, Dirichlet on every side.  k is 1 or
    `contrast` in a checkerboard of block^d cells; a face between two cells has the harmonic mean of their k, a boundary face 2 k."""
    shape = tuple(int(s) for s in shape)
    k = _block_checkerboard(shape, block, contrast)
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape)
    rows, cols, vals = [], [], []
    diag = np.zeros(shape)
    for d in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[d], hi[d] = slice(0, -1), slice(1, None)
        ka, kb = k[tuple(lo)], k[tuple(hi)]
        w = 2.0 * ka * kb / (ka + kb)
        a, b = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        rows += [a, b]
        cols += [b, a]
        vals += [-w.ravel(), -w.ravel()]
        diag[tuple(lo)] += w
        diag[tuple(hi)] += w
        first = [slice(None)] * len(shape)
        last = [slice(None)] * len(shape)
        first[d], last[d] = slice(0, 1), slice(-1, None)
        diag[tuple(first)] += 2.0 * k[tuple(first)]
        diag[tuple(last)] += 2.0 * k[tuple(last)]
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append(diag.ravel())
    return csr(sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)))


def nine_point_mixed(m: int, seed: int = 0) -> sp.csr_matrix:
    """A 9-point stencil that is SPD but not an M-matrix: the four axis neighbours -1, the NE/SW cross terms +0.5 and the NW/SE
    ones -0.5, diagonal 6.5 (strictly dominant); then D A D with D ~ U(0.5, 2) so that no two values are round."""
    n = m * m
    iy, ix = np.divmod(np.arange(n), m)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 6.5)]
    for dy, dx, v in ((0, 1, -1.0), (1, 0, -1.0), (1, 1, 0.5), (1, -1, -0.5)):
        ok = (iy + dy < m) & (ix + dx >= 0) & (ix + dx < m)
        a = np.nonzero(ok)[0]
        b = a + dy * m + dx
        rows += [a, b]
        cols += [b, a]
        vals += [np.full(a.size, v), np.full(a.size, v)]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    d = sp.diags(np.random.default_rng(seed).uniform(0.5, 2.0, n))
    return csr(d @ A @ d)


def random_bbt(n: int, per_row: int = 3, delta: float = 1e-2, seed: int = 0) -> sp.csr_matrix:
    """B B^T + delta I with B n x n, `per_row` random entries of random sign per row (values of both signs off the diagonal)."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = rng.integers(0, n, r.size)
    B = sp.csr_matrix((rng.standard_normal(r.size), (r, c)), shape=(n, n))
    A = csr(B @ B.T + delta * sp.identity(n))
    A.eliminate_zeros()
    return A


def with_identity_rows(A, rows) -> sp.csr_matrix:
    """A with the given rows replaced by identity rows; their couplings are dropped in the rows AND the columns (still symmetric)."""
    A = sp.csr_matrix(A, dtype=np.float64).tolil()
    for i in rows:
        A[i, :] = 0.0
        A[:, i] = 0.0
        A[i, i] = 1.0
    A = csr(A)
    A.eliminate_zeros()
    return A


def poisson2d(m: int) -> sp.csr_matrix:
    I = sp.identity(m, format="csr")
    return csr(sp.kron(I, _tri(m)) + sp.kron(_tri(m), I))


def poisson3d(m: int) -> sp.csr_matrix:
    I = sp.identity(m, format="csr")
    return csr(sp.kron(sp.kron(I, I), _tri(m)) + sp.kron(sp.kron(I, _tri(m)), I) + sp.kron(sp.kron(_tri(m), I), I))


def boundary_identity(m: int, every: int = 3) -> sp.csr_matrix:
    """The m x m 5-point Poisson grid with every `every`-th boundary node turned into an identity row."""
    iy, ix = np.divmod(np.arange(m * m), m)
    boundary = np.nonzero((iy == 0) | (ix == 0) | (iy == m - 1) | (ix == m - 1))[0]
    return with_identity_rows(poisson2d(m), boundary[::every])


def three_components() -> sp.csr_matrix:
    """Block diagonal of three unequal, differently scaled components: a 2-D grid, an anisotropic grid and a 3-D grid."""
    return csr(sp.block_diag([poisson2d(30), 1e3 * anisotropic2d(20, 1e-2), 0.5 * poisson3d(8)]))


def tiny_components(m: int = 24) -> sp.csr_matrix:
    """A 2-D grid with a component of 1 row and one of 2 rows after it."""
    return csr(sp.block_diag([poisson2d(m), sp.csr_matrix([[3.0]]), sp.csr_matrix([[2.0, -1.0], [-1.0, 2.0]])]))


def with_stored_zeros(A, seed: int = 0, frac: float = 0.5) -> sp.csr_matrix:
    """A plus explicit zeros kept in the CSR pattern: at a random `frac` of the symmetric positions (i, i + 2), (i, i + m + 1)
    that A does not hold (m = round(sqrt(n)))."""
    A = csr(A)
    n = A.shape[0]
    m = max(2, int(round(np.sqrt(n))))
    rng = np.random.default_rng(seed)
    zr, zc = [], []
    for off in (2, m + 1):
        a = np.arange(n - off)
        a = a[rng.random(a.size) < frac]
        zr += [a, a + off]
        zc += [a + off, a]
    zr, zc = np.concatenate(zr), np.concatenate(zc)
    present = np.asarray(A[zr, zc]).ravel() != 0
    zr, zc = zr[~present], zc[~present]
    C = A.tocoo()
    r = np.concatenate([C.row, zr])
    c = np.concatenate([C.col, zc])
    v = np.concatenate([C.data, np.zeros(zr.size)])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    return sp.csr_matrix((v, c.astype(np.int32), indptr), shape=(n, n))


def hub(m: int, k: int, delta: float = 1e-2, seed: int = 0) -> sp.csr_matrix:
    """Graph Laplacian + delta I of an m x m grid (unit weights) with one extra node, the last row, coupled to k distinct grid
    nodes with weights ~ U(0.5, 2).  Row k + 1 of A is the hub's: A T expands exactly k + 1 products there."""
    g = m * m
    n = g + 1
    rng = np.random.default_rng(seed)
    nb = np.sort(rng.choice(g, size=k, replace=False))
    w = rng.uniform(0.5, 2.0, k)
    iy, ix = np.divmod(np.arange(g), m)
    rows, cols, vals = [], [], []
    for ok, step in ((ix < m - 1, 1), (iy < m - 1, m)):
        a = np.nonzero(ok)[0]
        b = a + step
        rows += [a, b]
        cols += [b, a]
        vals += [-np.ones(a.size), -np.ones(a.size)]
    hubi = np.full(k, g)
    rows += [nb, hubi]
    cols += [hubi, nb]
    vals += [-w, -w]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    W = sp.csr_matrix((v, (r, c)), shape=(n, n))
    deg = -np.asarray(W.sum(axis=1)).ravel()
    return csr(W + sp.diags(deg + delta))


def tiny(n: int) -> sp.csr_matrix:
    """A 1-D Laplacian of n rows with a shifted diagonal (n = 1: [[3]])."""
    if n == 1:
        return csr(sp.csr_matrix([[3.0]]))
    return csr(_tri(n) + sp.identity(n))


def scaled_rows(A, lo: float = -8.0, hi: float = 8.0, seed: int = 0) -> sp.csr_matrix:
    """S A S with S = 10^U(lo, hi): row norms over 10^(2 lo) .. 10^(2 hi), the same pattern and still SPD."""
    s = 10.0 ** np.random.default_rng(seed).uniform(lo, hi, A.shape[0])
    return csr(sp.diags(s) @ csr(A) @ sp.diags(s))


def banded_spd(n: int, hb: int, seed: int = 0) -> sp.csr_matrix:
    """A full band of half-bandwidth hb (every |i - j| <= hb stored), off-diagonals ~ U(-1, 1), strictly diagonally dominant."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in range(1, hb + 1):
        a = np.arange(n - d)
        v = rng.uniform(-1.0, 1.0, a.size)
        v[v == 0.0] = 0.5
        rows += [a, a + d]
        cols += [a + d, a]
        vals += [v, v]
    W = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)) if rows else \
        sp.csr_matrix((n, n))
    dom = np.asarray(abs(W).sum(axis=1)).ravel()
    return csr(W + sp.diags(dom + 1.0))


def signed_ties(m: int, seed: int = 0) -> sp.csr_matrix:
    """The 5-point grid with off-diagonals +1 or -1 (symmetric, random sign per edge), diagonal 4.5: equal |values| of both signs,
    exactly representable, so the ILUT selections meet ties that only the column decides."""
    A = poisson2d(m).tocoo()
    rng = np.random.default_rng(seed)
    up = A.row < A.col
    sign = np.ones(A.nnz)
    s = rng.choice([-1.0, 1.0], int(up.sum()))
    key = {(int(r), int(c)): float(v) for r, c, v in zip(A.row[up], A.col[up], s)}
    for q in range(A.nnz):
        r, c = int(A.row[q]), int(A.col[q])
        if r != c:
            sign[q] = key[(min(r, c), max(r, c))]
    data = np.where(A.row == A.col, 4.5, sign)
    return csr(sp.coo_matrix((data, (A.row, A.col)), shape=A.shape))


def ilut_candidates(n_direct: int, n_fill: int = 60, n: int = 320, strong: int = 4) -> sp.csr_matrix:
    """A row (the last) whose ILUT working set holds n_direct + n_fill + 2 positions when nothing above tau_i = 0.01 ||row|| but
    `strong` of the direct couplings survives: node 0 is coupled to nodes 1 .. n_fill (its U row keeps them) and to the last
    node, whose elimination of column 0 therefore creates n_fill fill positions; the last row also holds n_direct small
    couplings to nodes n_fill + 1 .., of which the first `strong` are large enough to be kept."""
    last = n - 1
    assert n_fill + n_direct + 1 < last
    rows, cols, vals = [], [], []

    def add(i, j, v):
        rows.extend([i, j])
        cols.extend([j, i])
        vals.extend([v, v])
    for j in range(1, n_fill + 1):
        add(0, j, -0.5)
    add(0, last, -2.0)
    for t, j in enumerate(range(n_fill + 1, n_fill + 1 + n_direct)):
        add(last, j, -0.2 if t < strong else -1e-4 * (1 + (t % 7)))
    W = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    dom = np.asarray(abs(W).sum(axis=1)).ravel()
    return csr(W + sp.diags(dom + 1.0))


def product_counts(X, Y) -> np.ndarray:
    """Products row i of X Y expands in a row-wise SpGEMM: sum over the stored k of X[i, :] of nnz(Y[k, :]) (stored zeros count)."""
    X = sp.csr_matrix(X)
    Xb = sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    return np.rint(Xb @ np.diff(sp.csr_matrix(Y).indptr).astype(np.float64)).astype(np.int64)


def pattern_product(X, Y) -> sp.csr_matrix:
    """The structure a symbolic SpGEMM gives X Y: every column some product reaches, whatever the values (ones here)."""
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    Xb = sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    Yb = sp.csr_matrix((np.ones(Y.nnz), Y.indices, Y.indptr), shape=Y.shape)
    return (Xb @ Yb).tocsr()
