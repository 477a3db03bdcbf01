"""Plain numpy fp64 restatement of the training-path COO operators (k_batched_coo_spmv / _edge / _spmm / _sddmm in dpcg_setup.hip) and of
COO -> CSR (dpcg_coo.hip), written from the operations' definitions in include/dpcg.h.  Test infrastructure, not product.

The four operators work on triples (batch_k, row_k, col_k) with one feature each; (row, col) swap under `transpose`:

    spmv    out[b, row_k]    += feat[k] * vec[b, col_k]
    edge    out[k]            = a[b, row_k] * c[b, col_k]
    spmm    out[b, row_k, j] += feat[k] * panel[b, col_k, j]        j < ncols
    sddmm   out[k]            = sum_j g[b, row_k, j] * panel[b, col_k, j]

with the two guards of the kernels restated: a triple outside [0, batch) x [0, dof)^2 contributes nothing (spmv, spmm) or gives 0.0 (edge,
sddmm), and spmm -- spmm alone -- skips a triple whose feature is zero before it looks at the panel.

Each returns a `Result`: the fp64 value and, per output element, the number of terms that contribute (`m`), S = sum |term| and the smallest
non-zero |term|.  With fp32-exact operands every product is exact in fp64 (24 + 24 bits), so `value` carries only the rounding of an fp64
sum.  `Result.bound()` is the a-priori fp32 bound gamma_m * S, gamma_m = m u / (1 - m u), u = 2^-24: a sum of m products, each rounded once
(or fused into its addition) and added in ANY order, takes m - 1 additions and one product rounding per term on the longest path, at most m
roundings -- Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2.  Nothing in it is measured.

`skip` leaves terms out; the mutants of tests/test_coo_edges_host.py go through it.
"""

from __future__ import annotations

import dataclasses

import numpy as np

U = 2.0 ** -24


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


@dataclasses.dataclass
class Result:
    value: np.ndarray      # fp64
    m: np.ndarray          # int64: contributing terms per output
    S: np.ndarray          # fp64: sum of |term| per output (NaN where a term is NaN)
    smallest: np.ndarray   # fp64: the smallest non-zero finite |term| per output, inf where there is none

    def bound(self) -> np.ndarray:
        return gamma(self.m) * self.S


def _triples(idx, batch: int, dof: int, transpose: bool):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    b, r, c = idx[:, 0], idx[:, 2 if transpose else 1], idx[:, 1 if transpose else 2]
    ok = (b >= 0) & (b < batch) & (r >= 0) & (r < dof) & (c >= 0) & (c < dof)
    return b, r, c, ok


def _scattered(size: int, where: np.ndarray, terms: np.ndarray, shape) -> Result:
    """every term added to its output, in storage order"""
    value = np.bincount(where, weights=terms, minlength=size)
    m = np.bincount(where, minlength=size)
    mag = np.abs(terms)
    S = np.bincount(where, weights=mag, minlength=size)
    smallest = np.full(size, np.inf)
    counted = np.isfinite(mag) & (mag > 0)
    np.minimum.at(smallest, where[counted], mag[counted])
    return Result(value.reshape(shape), m.reshape(shape), S.reshape(shape), smallest.reshape(shape))


def spmv(idx, feat, vec, batch: int, dof: int, transpose: bool, skip=None) -> Result:
    b, r, c, ok = _triples(idx, batch, dof, transpose)
    if skip is not None:
        ok = ok & ~np.asarray(skip, dtype=bool)
    feat = np.asarray(feat, dtype=np.float64).reshape(-1)
    vec = np.asarray(vec, dtype=np.float64).reshape(batch, dof)
    b, r, c = b[ok], r[ok], c[ok]
    with np.errstate(invalid="ignore"):
        terms = feat[ok] * vec[b, c]                     # no zero test: 0 * inf = NaN, as IEEE has it
    return _scattered(batch * dof, b * dof + r, terms, (batch, dof))


def edge(idx, a, c, batch: int, dof: int, transpose: bool, skip=None) -> Result:
    b, r, cc, ok = _triples(idx, batch, dof, transpose)
    if skip is not None:
        ok = ok & ~np.asarray(skip, dtype=bool)
    a = np.asarray(a, dtype=np.float64).reshape(batch, dof)
    c = np.asarray(c, dtype=np.float64).reshape(batch, dof)
    value = np.zeros(len(b))
    with np.errstate(invalid="ignore"):
        value[ok] = a[b[ok], r[ok]] * c[b[ok], cc[ok]]
    mag = np.abs(value)
    return Result(value, ok.astype(np.int64), mag, np.where(np.isfinite(mag) & (mag > 0), mag, np.inf))


def spmm(idx, feat, panel, batch: int, dof: int, ncols: int, transpose: bool, skip=None) -> Result:
    b, r, c, ok = _triples(idx, batch, dof, transpose)
    feat = np.asarray(feat, dtype=np.float64).reshape(-1)
    ok = ok & (feat != 0.0)                              # the zero guard (+0 and -0): the panel row is not looked at
    panel = np.asarray(panel, dtype=np.float64).reshape(batch, dof, ncols)
    keep = np.broadcast_to(ok[:, None], (len(b), ncols)).copy()
    if skip is not None:
        skip = np.asarray(skip, dtype=bool)
        keep &= ~(skip if skip.ndim == 2 else skip[:, None])
    k, j = np.nonzero(keep)
    terms = feat[k] * panel[b[k], c[k], j]
    return _scattered(batch * dof * ncols, (b[k] * dof + r[k]) * ncols + j, terms, (batch, dof, ncols))


def sddmm(idx, g, panel, batch: int, dof: int, ncols: int, transpose: bool, skip=None) -> Result:
    b, r, c, ok = _triples(idx, batch, dof, transpose)
    g = np.asarray(g, dtype=np.float64).reshape(batch, dof, ncols)
    panel = np.asarray(panel, dtype=np.float64).reshape(batch, dof, ncols)
    keep = np.broadcast_to(ok[:, None], (len(b), ncols)).copy()
    if skip is not None:
        skip = np.asarray(skip, dtype=bool)
        keep &= ~(skip if skip.ndim == 2 else skip[:, None])
    terms = np.zeros((len(b), ncols))
    with np.errstate(invalid="ignore"):
        terms[ok] = g[b[ok], r[ok]] * panel[b[ok], c[ok]]
    terms = np.where(keep, terms, 0.0)
    mag = np.abs(terms)
    counted = keep & np.isfinite(mag) & (mag > 0)
    smallest = np.where(counted, mag, np.inf).min(axis=1, initial=np.inf)
    return Result(terms.sum(axis=1), keep.sum(axis=1).astype(np.int64), mag.sum(axis=1), smallest)


def coo_to_csr(rows, cols, vals, n: int, stable: bool = True):
    """(rowptr int32[n + 1], col int32[unique], val fp64[unique]): a stable sort by (row, col), then each run of equal keys added
    up in storage order, one fp64 addition after the other.  stable=False is the mutant: equal keys come out back to front."""
    rows = [int(v) for v in np.asarray(rows).reshape(-1)]
    cols = [int(v) for v in np.asarray(cols).reshape(-1)]
    vals = [float(v) for v in np.asarray(vals, dtype=np.float64).reshape(-1)]
    if not (len(rows) == len(cols) == len(vals)):
        raise ValueError("rows, cols, vals must have the same length")
    if n <= 0 or any(r < 0 or r >= n for r in rows) or any(c < 0 or c >= n for c in cols):
        raise ValueError("index out of range")
    if stable:
        order = sorted(range(len(rows)), key=lambda k: (rows[k], cols[k]))        # Python's sort is stable
    else:
        order = sorted(range(len(rows)), key=lambda k: (rows[k], cols[k], -k))
    count = [0] * (n + 1)
    col_out, val_out = [], []
    last = None
    for k in order:
        key = (rows[k], cols[k])
        if key == last:
            val_out[-1] = val_out[-1] + vals[k]
        else:
            col_out.append(cols[k])
            val_out.append(vals[k])
            count[rows[k] + 1] += 1
            last = key
    return (np.cumsum(count).astype(np.int32), np.asarray(col_out, dtype=np.int32).reshape(-1),
            np.asarray(val_out, dtype=np.float64).reshape(-1))
