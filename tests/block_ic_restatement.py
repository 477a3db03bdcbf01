"""Numpy restatement of the block-Jacobi incomplete Cholesky (dpcg_set_precond_block_ic, include/dpcg.h): the contract the device
factor and apply equal bit for bit.

Numbering: rows sorted stably by (block id, caller's row); perm[k] = the caller's row at factor position k; blocks = the maximal runs
of equal id.  A_B = P A P^T without the entries whose row and column lie in different blocks.  IC(0): oracle.ic0(A_B).  DIC:
d_i = a_ii - sum a_ij a_ij / d_j over the stored j < i ascending (one product, one division, one subtraction per term),
L_ij = a_ij / sqrt(d_j), L_ii = sqrt(d_i).  Apply: z = P^T L^-T L^-1 P r through oracle.sptrsv_lower / sptrsv_upper_t.

`fast=True` takes the compiled twins of the oracle's loops (oracle.c_oracle: the same operation order, pinned against oracle.oracle
by tests/test_oracle_golden.py and, for this use, by tests/test_block_ic_host.py) where the Python loops would take minutes."""

import numpy as np
import scipy.sparse as sp

from oracle import oracle as O


def numbering(block_of_row):
    ids = np.asarray(block_of_row)
    return np.argsort(ids, kind="stable").astype(np.int32)


def contiguous_ids(n, block_rows):
    return (np.arange(n, dtype=np.int64) // int(block_rows)).astype(np.int32)


def block_matrix(A, block_of_row):
    """A_B in the factor numbering (CSR, sorted columns)."""
    ids = np.asarray(block_of_row)
    perm = numbering(ids)
    A = sp.csr_matrix(A, dtype=np.float64)
    C = A[perm][:, perm].tocoo()
    s = ids[perm]
    keep = s[C.row] == s[C.col]
    B = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)
    B.sort_indices()
    return B


def dic(AB):
    T = sp.tril(AB, format="csr")
    T.sort_indices()
    rp, ci = T.indptr, T.indices
    a = T.data.astype(np.float64)
    n = T.shape[0]
    d = np.zeros(n)
    for i in range(n):
        e = rp[i + 1] - 1
        assert ci[e] == i, f"missing diagonal at factor row {i}"
        acc = a[e]
        for k in range(rp[i], e):
            t = a[k] * a[k]
            t = t / d[ci[k]]
            acc = acc - t
        if not (acc > 0.0 and np.isfinite(acc)):
            raise ArithmeticError(f"DIC breakdown at factor row {i}")
        d[i] = acc
    s = np.sqrt(d)
    lv = a.copy()
    for i in range(n):
        e = rp[i + 1] - 1
        for k in range(rp[i], e):
            lv[k] = a[k] / s[ci[k]]
        lv[e] = s[i]
    return sp.csr_matrix((lv, ci.copy(), rp.copy()), shape=T.shape)


def factor(A, block_of_row, variant="ic0", fast=False):
    """(L, perm): the factor in the factor numbering (int32 CSR, diagonal last in a row) and the numbering."""
    AB = block_matrix(A, block_of_row)
    if variant == "dic":
        L = dic(AB)
    elif fast:
        from oracle import c_oracle as CO
        L = CO.ic0(AB)
    else:
        L = O.ic0(AB)
    L = sp.csr_matrix(L)
    L.indices, L.indptr = L.indices.astype(np.int32), L.indptr.astype(np.int32)
    return L, numbering(block_of_row)


def apply(L, perm, r, fast=False):
    r = np.asarray(r, dtype=np.float64)
    if fast:
        from oracle import c_oracle as CO
        y = CO.sptrsv_upper(CO.transpose_csr(L), CO.sptrsv_lower(L, r[perm]))
    else:
        y = O.sptrsv_upper_t(L, O.sptrsv_lower(L, r[perm]))
    z = np.empty_like(y)
    z[perm] = y
    return z


class Apply:
    """M as `M @ r` for oracle.preconditioned_conjugate_gradient."""

    def __init__(self, L, perm, fast=True):
        self.L, self.perm, self.fast = L, perm, fast

    def __matmul__(self, r):
        return apply(self.L, self.perm, r, fast=self.fast)


def _levels(T, upper):
    n = T.shape[0]
    rp, ci = T.indptr, T.indices
    lev = np.zeros(n, dtype=np.int64)
    rows = range(n - 1, -1, -1) if upper else range(n)
    for i in rows:
        m = -1
        for k in range(rp[i], rp[i + 1]):
            if ci[k] != i:
                m = max(m, lev[ci[k]])
        lev[i] = m + 1
    return lev


def block_levels(L, block_of_row):
    """(most levels of L in any block, the same for L^T); L is block diagonal, so a block's levels are those of its rows."""
    ids = np.asarray(block_of_row)
    s = ids[numbering(ids)]
    Lc = sp.csr_matrix(L)
    Lt = sp.csr_matrix(Lc.T)
    Lt.sort_indices()
    lo, up = _levels(Lc, False), _levels(Lt, True)
    heads = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    return (int(np.maximum.reduceat(lo, heads).max()) + 1, int(np.maximum.reduceat(up, heads).max()) + 1)


def dense_m(L, perm):
    """M = P^T (L L^T)^-1 P as a dense matrix (small n)."""
    n = L.shape[0]
    Ld = L.toarray()
    Minv = np.linalg.inv(Ld @ Ld.T)
    P = np.zeros((n, n))
    P[np.arange(n), perm] = 1.0
    return P.T @ Minv @ P
