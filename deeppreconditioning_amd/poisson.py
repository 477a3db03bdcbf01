"""Synthetic pressure-Poisson systems generated directly in HBM.

The reference cannot produce the 1M-DoF / 256^3 systems BASELINE.json names (its matrices come out
of OpenFOAM as dense lists, foam/newInterFoam/pEqn.H:54-68), so they are synthesised: closed-form
5-point / 7-point Laplacians, kron(I,T)+kron(T,I)[+...] with T = tridiag(-1,2,-1).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .operators import CsrSystem, _dev_ptr, _stream


def poisson_sizes(dim: int, n: int) -> tuple[int, int]:
    rows, nnz = C.c_int64(), C.c_int64()
    L.check(L.lib().dpcg_poisson_sizes(dim, n, C.byref(rows), C.byref(nnz)))
    return rows.value, nnz.value


def poisson_csr(dim: int, n: int, device=None, dtype=torch.float64):
    """(rowptr, col, val) CUDA tensors of the dim-D Poisson matrix on an n^dim grid."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    rows, nnz = poisson_sizes(dim, n)
    rowptr = torch.empty(rows + 1, dtype=torch.int32, device=device)
    col = torch.empty(nnz, dtype=torch.int32, device=device)
    val = torch.empty(nnz, dtype=dtype, device=device)
    with torch.cuda.device(device):
        L.check(L.lib().dpcg_gen_poisson(dim, n, _dev_ptr(rowptr), _dev_ptr(col), _dev_ptr(val),
                                         L.F64 if dtype == torch.float64 else L.F32, _stream()))
    return rowptr, col, val


def poisson_system(dim: int, n: int, device=None, dtype=torch.float64) -> CsrSystem:
    rowptr, col, val = poisson_csr(dim, n, device, dtype)
    return CsrSystem(rowptr, col, val, rowptr.numel() - 1)


def rhs(n: int, seed: int = 0, device=None) -> torch.Tensor:
    """b ~ U(-1,1) as generate_data.py:106, seeded like the golden fixtures (`default_rng(seed)`)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, n)).to(device)


def neumann_csr(dims, coefficient_seed=None):
    """Host-side pure-Neumann pressure matrix of a closed box: the 5-point (len(dims) == 2) or 7-point (3) graph Laplacian of a
    dims[0] x dims[1] [x dims[2]] grid, first index fastest -- a_ij = -w_ij for neighbours, a_ii = the sum of the row's weights, so
    every row sums to zero: symmetric positive SEMI-definite, its null space the constants (`CsrSystem.set_nullspace("constant")`).
    `coefficient_seed`: None gives unit weights; an int draws one weight 10^U(-1, 1) per edge from `default_rng(seed)`, axis by
    axis in row order (a variable-coefficient, e.g. two-phase, system).  Returns a scipy CSR matrix with sorted int32 indices."""
    import scipy.sparse as sp
    dims = tuple(int(d) for d in dims)
    if len(dims) not in (2, 3) or min(dims) < 1:
        raise ValueError("dims must be 2 or 3 positive grid sizes")
    rows = int(np.prod(dims))
    idx = np.arange(rows, dtype=np.int64)
    rng = None if coefficient_seed is None else np.random.default_rng(coefficient_seed)
    r_list, c_list, v_list = [], [], []
    diag = np.zeros(rows)
    off = 1
    for d in dims:
        lo = idx[(idx // off) % d < d - 1]            # the lower end of every edge along this axis
        w = np.ones(lo.size) if rng is None else 10.0 ** rng.uniform(-1.0, 1.0, lo.size)
        r_list += [lo, lo + off]
        c_list += [lo + off, lo]
        v_list += [-w, -w]
        np.add.at(diag, lo, w)
        np.add.at(diag, lo + off, w)
        off *= d
    r_list.append(idx)
    c_list.append(idx)
    v_list.append(diag)
    A = sp.csr_matrix((np.concatenate(v_list), (np.concatenate(r_list), np.concatenate(c_list))), shape=(rows, rows))
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def convection_diffusion_csr(shape, peclet, coefficient_seed=None):
    """Host-side first-order-upwind finite-volume convection-diffusion matrix on a shape[0] x shape[1] [x shape[2]] grid of unit
    cells, first index fastest: a structurally symmetric 5-point (2-D) or 7-point (3-D) pattern with NON-symmetric values -- what
    OpenFOAM's momentum and phase-fraction matrices look like, and what `CsrSystem.solve_bicgstab` is for.  Every face carries a
    diffusion coefficient d_f drawn from [1, 2) (`default_rng(coefficient_seed)`, None meaning seed 0; axis by axis: the interior
    faces in row order, then the faces on the lower boundary, then those on the upper one), so 1/diag is not a scalar.  A constant
    flux F = `peclet` >= 0 crosses every face in the positive direction of every axis (the cell Peclet number F / d_f lies in
    (peclet / 2, peclet]).  Across the face between cell i and its upper neighbour j: a_ii += d_f + F, a_ij = -d_f,
    a_ji = -(d_f + F), a_jj += d_f.  Dirichlet boundaries (value 0 on the boundary face): a_ii += d_f on both, and a_ii += F on the
    outflow side.  Off-diagonals are negative, every row is weakly and every boundary row strictly diagonally dominant: a
    nonsingular M-matrix.  peclet = 0 gives a symmetric variable-coefficient Poisson matrix.  Returns a scipy CSR matrix with sorted
    int32 indices."""
    import scipy.sparse as sp
    shape = tuple(int(d) for d in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError("shape must be 2 or 3 positive grid sizes")
    flux = float(peclet)
    if not (flux >= 0.0 and np.isfinite(flux)):
        raise ValueError("peclet must be finite and >= 0")
    rows = int(np.prod(shape))
    idx = np.arange(rows, dtype=np.int64)
    rng = np.random.default_rng(0 if coefficient_seed is None else coefficient_seed)
    r_list, c_list, v_list = [], [], []
    diag = np.zeros(rows)
    off = 1
    for d in shape:
        pos = (idx // off) % d
        lo = idx[pos < d - 1]                         # the lower cell of every interior face along this axis
        w = rng.uniform(1.0, 2.0, lo.size)
        r_list += [lo, lo + off]
        c_list += [lo + off, lo]
        v_list += [-w, -(w + flux)]
        np.add.at(diag, lo, w + flux)
        np.add.at(diag, lo + off, w)
        first, last = idx[pos == 0], idx[pos == d - 1]
        np.add.at(diag, first, rng.uniform(1.0, 2.0, first.size))
        np.add.at(diag, last, rng.uniform(1.0, 2.0, last.size) + flux)
        off *= d
    r_list.append(idx)
    c_list.append(idx)
    v_list.append(diag)
    A = sp.csr_matrix((np.concatenate(v_list), (np.concatenate(r_list), np.concatenate(c_list))), shape=(rows, rows))
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def _subdomain_boxes(shape, blocks):
    """(box id per grid point, number of boxes) of the box partition `subdomain_indicators` and `subdomain_blocks` share."""
    shape = tuple(int(d) for d in shape)
    blocks = tuple(int(d) for d in blocks)
    if len(shape) != len(blocks) or not shape or min(shape) < 1 or min(blocks) < 1:
        raise ValueError("shape and blocks need the same number of positive entries")
    if any(nb > d for d, nb in zip(shape, blocks)):
        raise ValueError("a block would be empty: more blocks than grid points along an axis")
    rows = int(np.prod(shape))
    idx = np.arange(rows, dtype=np.int64)
    box = np.zeros(rows, dtype=np.int64)
    off, boff = 1, 1
    for d, nb in zip(shape, blocks):
        box += ((idx // off) % d) * nb // d * boff         # point c of the axis lies in run floor(c nb / d)
        off *= d
        boff *= nb
    return box, int(np.prod(blocks))


def subdomain_blocks(shape, blocks):
    """The box id of every grid point, (prod(shape),) int32, for the box partition of `subdomain_indicators` (the same cut rule:
    axis a into blocks[a] runs of near-equal length, box ids with the first axis fastest) -- the `blocks=` of `BlockIC`."""
    return _subdomain_boxes(shape, blocks)[0].astype(np.int32)


def subdomain_indicators(shape, blocks):
    """The piecewise-constant deflation vectors of a box partition (Nicolaides' subdomain deflation; `CsrSystem.set_deflation`): the
    grid `shape` (first index fastest, as `neumann_csr` and `poisson_csr` number it) is cut into blocks[0] x blocks[1] [x ...] boxes,
    axis a into blocks[a] runs of near-equal length, and column j of the (prod(shape), prod(blocks)) result is 1 on box j and 0
    elsewhere -- every row sums to 1.  ValueError when a box would be empty (more blocks than grid points along an axis)."""
    box, n_boxes = _subdomain_boxes(shape, blocks)
    W = np.zeros((box.size, n_boxes), order="F")
    W[np.arange(box.size, dtype=np.int64), box] = 1.0
    return W


def unstructured_like_csr(dim: int, n: int, seed: int = 0):
    """Host-side stand-in for an OpenFOAM pressure matrix: D (P A P^T) D of the
    Poisson matrix with a seeded random symmetric permutation P and D = diag(U(0.5, 2)).  Returns a scipy CSR
    matrix with sorted int32 indices (setup-time plumbing; the solve never touches the host copy)."""
    import scipy.sparse as sp
    rows, nnz = poisson_sizes(dim, n)
    idx = np.arange(rows, dtype=np.int64)
    offs = [1, n] if dim == 2 else [1, n, n * n]
    coords = [idx % n, (idx // n) % n] if dim == 2 else [idx % n, (idx // n) % n, idx // (n * n)]
    r_list, c_list, v_list = [idx], [idx], [np.full(rows, 2.0 * dim)]
    for off, co in zip(offs, coords):
        ok = co < n - 1
        r_list += [idx[ok], idx[ok] + off]
        c_list += [idx[ok] + off, idx[ok]]
        v_list += [np.full(int(ok.sum()), -1.0)] * 2
    rng = np.random.default_rng(seed)
    perm = rng.permutation(rows)
    d = rng.uniform(0.5, 2.0, rows)
    inv = np.empty(rows, dtype=np.int64)
    inv[perm] = idx                                   # B[i, j] = A[perm[i], perm[j]]
    r = inv[np.concatenate(r_list)]
    c = inv[np.concatenate(c_list)]
    v = np.concatenate(v_list) * d[r] * d[c]
    B = sp.csr_matrix((v, (r, c)), shape=(rows, rows))
    B.sort_indices()
    B.indices = B.indices.astype(np.int32)
    B.indptr = B.indptr.astype(np.int32)
    assert B.nnz == nnz
    return B
