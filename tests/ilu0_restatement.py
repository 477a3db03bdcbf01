"""numpy restatement of dpcg_set_precond_ilu0 (include/dpcg.h): ILU(0) and DILU on the pattern of A, row loops, one rounding per
operation (the library is compiled with -ffp-contract=off).  The device factors equal these bit for bit.

    ilu0(A)  rows i ascending, on the pattern of A with sorted rows: for each stored k < i, ascending, l_ik = a_ik / u_kk; then for
             each stored (k, j), j > k, ascending: if (i, j) is stored, a_ij = a_ij - l_ik * u_kj.  Every entry receives its
             subtractions in ascending k.
    dilu(A)  OpenFOAM's rule: d_i = a_ii; for each stored k < i, ascending, for which (k, i) is stored too: t = a_ik * a_ki;
             t = t / d_k; d_i = d_i - t.  L = I + strict_lower(A) D^-1 (l_ik = a_ik / d_k), U = D + strict_upper(A).

Both return (L, U) as scipy CSR whose arrays are laid out as the device's: L the strict lower part with a unit diagonal stored LAST in
every row, U with the diagonal FIRST; columns ascending.  A missing diagonal raises MissingDiagonal, a pivot that is zero or not
finite raises BadPivot(row) for the first such row.
"""

import numpy as np
import scipy.sparse as sp


class MissingDiagonal(ValueError):
    pass


class BadPivot(ValueError):
    def __init__(self, row):
        super().__init__(f"zero or non-finite pivot at row {row}")
        self.row = row


def _sorted_rows(A):
    A = sp.csr_matrix(A, dtype=np.float64, copy=True)
    A.sort_indices()
    n = A.shape[0]
    rp, ci, v = A.indptr, A.indices, A.data
    dpos = np.empty(n, dtype=np.int64)
    for i in range(n):
        hit = np.nonzero(ci[rp[i]:rp[i + 1]] == i)[0]
        if hit.size == 0:
            raise MissingDiagonal(f"missing diagonal entry at row {i}")
        dpos[i] = rp[i] + hit[0]
    return n, rp, ci, v, dpos


def _split(n, rp, ci, v, dpos):
    """(L, U) in the device's layout from the worked-on values: strict lower + a unit diagonal last, diagonal first + strict upper"""
    lrp, urp = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    lci, lv, uci, uv = [], [], [], []
    for i in range(n):
        lo = slice(rp[i], dpos[i])
        up = slice(dpos[i], rp[i + 1])
        lci.extend(ci[lo]); lv.extend(v[lo]); lci.append(i); lv.append(1.0)
        uci.extend(ci[up]); uv.extend(v[up])
        lrp[i + 1], urp[i + 1] = len(lci), len(uci)
    mk = lambda val, col, ptr: sp.csr_matrix((np.array(val, dtype=np.float64), np.array(col, dtype=np.int32), ptr), shape=(n, n))
    return mk(lv, lci, lrp), mk(uv, uci, urp)


def _check_pivot(d, i):
    if d == 0.0 or not np.isfinite(d):
        raise BadPivot(i)


def ilu0(A):
    n, rp, ci, v, dpos = _sorted_rows(A)
    with np.errstate(all="ignore"):
        for i in range(n):
            for a in range(rp[i], dpos[i]):
                k = ci[a]
                l = v[a] / v[dpos[k]]
                v[a] = l
                pos = a + 1                                    # (both rows ascend: row i is searched forward only)
                for b in range(dpos[k] + 1, rp[k + 1]):
                    j = ci[b]
                    while pos < rp[i + 1] and ci[pos] < j:
                        pos += 1
                    if pos < rp[i + 1] and ci[pos] == j:
                        p = l * v[b]
                        v[pos] = v[pos] - p
            _check_pivot(v[dpos[i]], i)
    return _split(n, rp, ci, v, dpos)


def dilu(A):
    n, rp, ci, v, dpos = _sorted_rows(A)
    d = np.empty(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            di = v[dpos[i]]
            for a in range(rp[i], dpos[i]):
                k = ci[a]
                for b in range(dpos[k] + 1, rp[k + 1]):
                    if ci[b] == i:
                        t = v[a] * v[b]
                        t = t / d[k]
                        di = di - t
                        break
            d[i] = di
            _check_pivot(di, i)
        for i in range(n):
            for a in range(rp[i], dpos[i]):
                v[a] = v[a] / d[ci[a]]
            v[dpos[i]] = d[i]
    return _split(n, rp, ci, v, dpos)


FACTOR = {"ilu0": ilu0, "dilu": dilu}


def permuted(A, perm):
    """Q A Q^T with sorted rows: row k of the result is row perm[k] of A"""
    perm = np.asarray(perm)
    B = sp.csr_matrix(A)[perm][:, perm].tocsr()
    B.sort_indices()
    return B


def red_black(shape):
    """perm of the two-colour ordering of a grid whose first index runs fastest (cells by the parity of the sum of their indices, each
    colour in the caller's order)"""
    idx = np.indices(shape).sum(axis=0).ravel(order="F") % 2
    return np.concatenate([np.nonzero(idx == 0)[0], np.nonzero(idx == 1)[0]]).astype(np.int32)


def lu_solve_apply(Lf, Uf, perm=None):
    """v -> Q^T U^-1 L^-1 Q v by substitution (perm None: Q = I)"""
    import scipy.sparse.linalg as spla
    Lc, Uc = sp.csr_matrix(Lf, copy=True), sp.csr_matrix(Uf, copy=True)       # (the caller's arrays keep their layout)
    Lc.sort_indices()
    Uc.sort_indices()
    if perm is None:
        return lambda v: spla.spsolve_triangular(Uc, spla.spsolve_triangular(Lc, v, lower=True, unit_diagonal=True), lower=False)
    perm = np.asarray(perm)

    def apply(v):
        z = np.empty_like(v)
        z[perm] = spla.spsolve_triangular(Uc, spla.spsolve_triangular(Lc, v[perm], lower=True, unit_diagonal=True), lower=False)
        return z
    return apply
