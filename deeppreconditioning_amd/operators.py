"""GPU operators behind the reference's duck-typed `A @ v` / `M @ v` protocol (cg.py:60,61,75,81).

`CsrSystem` owns a libdpcg handle for the system matrix A; the preconditioner classes describe how
`M @ r` is applied (test.py:70-105).  All arithmetic happens in the hand-written HIP kernels of
libdpcg.so; torch is used for device memory and streams only.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L

try:  # scipy is optional plumbing for host-side CSR inputs
    import scipy.sparse as _sp
except Exception:  # pragma: no cover
    _sp = None


# --------------------------------------------------------------------------------------------
# input normalisation (host logic, no GPU needed)
# --------------------------------------------------------------------------------------------
def _is_scipy(A) -> bool:
    return _sp is not None and _sp.issparse(A)


def csr_arrays(A):
    """Normalise a matrix-like to CSR parts: (space, rowptr, col, val, n).

    space = "host": numpy int32/int32/float64 arrays.  space = "device": torch CUDA tensors.
    Accepts scipy sparse, numpy 2-D, torch sparse-CSR / sparse-COO / dense tensors (the reference's
    callers pass DENSE fp64 tensors, test.py:61-68, train.py:93-95).  Columns ascend within a row.
    """
    if isinstance(A, tuple) and len(A) == 3:  # ready-made CSR parts (rowptr, col, val)
        rp, ci, v = A
        if isinstance(v, torch.Tensor):
            if v.is_cuda:
                return ("device", rp.to(torch.int32).contiguous(), ci.to(torch.int32).contiguous(),
                        v.to(torch.float64).contiguous(), rp.numel() - 1)
            rp, ci, v = rp.numpy(), ci.numpy(), v.numpy()
        return ("host", np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32),
                np.ascontiguousarray(v, dtype=np.float64), len(rp) - 1)
    if _is_scipy(A):
        M = A.tocsr()
        if not M.has_canonical_format:
            M = M.copy()
            M.sum_duplicates()
        return ("host", np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32),
                np.ascontiguousarray(M.data, dtype=np.float64), M.shape[0])
    if isinstance(A, np.ndarray):
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("expected a square 2-D array")
        return csr_arrays(_sp.csr_matrix(A))
    if isinstance(A, torch.Tensor):
        if A.dim() != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("expected a square 2-D tensor")
        if A.layout != torch.sparse_csr:
            A = A.to_sparse_csr() if A.layout == torch.strided else A.coalesce().to_sparse_csr()
        rp, ci, v = A.crow_indices(), A.col_indices(), A.values()
        if A.is_cuda:
            return ("device", rp.to(torch.int32).contiguous(), ci.to(torch.int32).contiguous(),
                    v.to(torch.float64).contiguous(), A.shape[0])
        return ("host", np.ascontiguousarray(rp.numpy(), dtype=np.int32), np.ascontiguousarray(ci.numpy(), dtype=np.int32),
                np.ascontiguousarray(v.to(torch.float64).numpy()), A.shape[0])
    raise TypeError(f"cannot interpret {type(A).__name__} as a sparse system matrix")


def diagonal_only(rowptr, col, n) -> bool:
    """True when the CSR pattern is exactly one entry (i, i) per row -- M = diag(d) (test.py:74-79)."""
    if isinstance(rowptr, torch.Tensor):
        if rowptr.numel() != n + 1 or col.numel() != n:
            return False
        ar = torch.arange(n + 1, device=rowptr.device, dtype=rowptr.dtype)
        return bool(torch.equal(rowptr, ar) and torch.equal(col, ar[:-1]))
    return len(col) == n and np.array_equal(rowptr, np.arange(n + 1)) and np.array_equal(col, np.arange(n))


def _dev_ptr(t: torch.Tensor | None, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("expected a CUDA (ROCm) tensor")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return C.c_void_p(t.data_ptr())


def _int32_indices(t, device, what: str) -> torch.Tensor:
    """`t` as a contiguous int32 tensor on `device`.  A value that does not fit int32 raises ValueError: `.to(torch.int32)` alone
    wraps it (3 + 2**32 becomes the valid index 3).  int32 input, the hot path, is not inspected."""
    is_tensor = isinstance(t, torch.Tensor)
    if not is_tensor:
        t = np.asarray(t)
    narrow = t.dtype == (torch.int32 if is_tensor else np.dtype(np.int32))
    if not narrow and (t.numel() if is_tensor else t.size) > 0:
        lo, hi = (int(v) for v in (torch.aminmax(t) if is_tensor else (t.min(), t.max())))
        if lo < -2 ** 31 or hi > 2 ** 31 - 1:
            raise ValueError(f"{what}: an index in [{lo}, {hi}] does not fit int32")
    if not is_tensor:
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32))
    return t.to(device=device, dtype=torch.int32).contiguous()


def _np_ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to_device_f64(v, device) -> torch.Tensor:
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.to(device=device, dtype=torch.float64).contiguous()


# --------------------------------------------------------------------------------------------
# preconditioner descriptions (how `M @ r` is applied)
# --------------------------------------------------------------------------------------------
class Preconditioner:
    """Base: a description that `CsrSystem.set_preconditioner` turns into libdpcg state.

    Instances also work stand-alone as duck-typed operators (`M @ r`), so they drop into an
    unmodified copy of the reference loop; that path builds a private handle on first use.
    """

    _private: "CsrSystem | None" = None

    def _attach(self, system: "CsrSystem") -> None:
        raise NotImplementedError

    def _private_system(self) -> "CsrSystem":
        raise NotImplementedError

    def __matmul__(self, r: torch.Tensor) -> torch.Tensor:
        if self._private is None:
            self._private = self._private_system()
            self._attach(self._private)
        return self._private.precond_apply(r)


class Identity(Preconditioner):
    """M = I, the `vanilla` technique (test.py:70-72)."""

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_none(system._h))

    def __matmul__(self, r):
        return r.clone()


class Jacobi(Preconditioner):
    """M = diag(1/a_ii) (test.py:74-79).  `dinv=None` extracts the diagonal of A on the device."""

    def __init__(self, dinv=None):
        self.dinv = dinv

    def _attach(self, system):
        if self.dinv is None:
            L.check(L.lib().dpcg_set_precond_jacobi(system._h, None, L.DEVICE, _stream()))
        else:
            d = _to_device_f64(self.dinv, system.device)
            if d.numel() != system.n:
                raise ValueError("dinv has the wrong length")
            L.check(L.lib().dpcg_set_precond_jacobi(system._h, _dev_ptr(d), L.DEVICE, _stream()))

    def _private_system(self):
        if self.dinv is None:
            raise ValueError("a stand-alone Jacobi operator needs explicit dinv")
        d = _to_device_f64(self.dinv, torch.device("cuda", torch.cuda.current_device()))
        n = d.numel()
        ar = torch.arange(n + 1, device=d.device, dtype=torch.int32)
        return CsrSystem(ar, ar[:-1].clone(), torch.ones(n, device=d.device, dtype=torch.float64), n)


class _CsrBacked(Preconditioner):
    def __init__(self, matrix):
        self.space, self.rowptr, self.col, self.val, self.n = csr_arrays(matrix)

    def _parts(self):
        if self.space == "host":
            return L.HOST, _np_ptr(self.rowptr), _np_ptr(self.col), _np_ptr(self.val), len(self.col)
        return L.DEVICE, _dev_ptr(self.rowptr), _dev_ptr(self.col), _dev_ptr(self.val), self.col.numel()

    def _private_system(self):
        if self.space == "host":
            return CsrSystem.from_host(self.rowptr, self.col, self.val, self.n)
        return CsrSystem(self.rowptr, self.col, self.val, self.n)


class CsrPreconditioner(_CsrBacked):
    """z = M r with M an explicit CSR matrix -- what test.py:88,105 hand to the solver (M = L L^T)."""

    def _attach(self, system):
        if self.n != system.n:
            raise ValueError("preconditioner size mismatch")
        space, rp, ci, v, nnz = self._parts()
        L.check(L.lib().dpcg_set_precond_csr(system._h, nnz, rp, ci, v, space, _stream()))


class LLtMultiply(_CsrBacked):
    """z = L (L^T r): the learned preconditioner of test.py:100-105 without forming L L^T."""

    mode = L.PRECOND_LLT_MULTIPLY

    def __init__(self, lower):
        super().__init__(lower)

    def _attach(self, system):
        if self.n != system.n:
            raise ValueError("factor size mismatch")
        space, rp, ci, v, nnz = self._parts()
        L.check(L.lib().dpcg_set_precond_llt(system._h, self.mode, nnz, rp, ci, v, space, _stream()))


class LLtSolve(LLtMultiply):
    """z = L^-T (L^-1 r): a true incomplete-Cholesky apply by level-scheduled triangular solves.

    The parallelism of a triangular solve is the width of the factor's dependency levels (`CsrSystem.info()`:
    `levels_lower` / `levels_upper`).  The factor of a grid has n^(1/2) .. n^(2/3)-row levels; a factor whose every row
    reaches back to its predecessor -- the sparsity the reference's CNN emits: 15 entries per row with column row-1 among
    them -- is ONE chain of n levels and is solved row after row (256^2: 65 536 levels, ~0.1 s per apply).  That factor is
    meant to be multiplied (`LLtMultiply`, the reference's own use, test.py:100-105)."""

    mode = L.PRECOND_LLT_SOLVE


class IC0(Preconditioner):
    """IC(0) of A computed at setup (stands in for ilupp.ichol0, test.py:83).

    mode="solve" applies it by triangular solves; mode="multiply" reproduces the reference's
    `_construct_incomplete_cholesky`, which multiplies by L L^T (test.py:88, marked unstable at
    test.py:45).

    ordering="multicolor" (solve mode): IC(0) of the matrix with its unknowns listed colour by colour (red-black for
    every 5- / 7-point grid) -- a DIFFERENT preconditioner from the reference's (another elimination order, ~+20 %
    iterations) whose two triangular solves are a handful of wide parallel sweeps instead of hundreds of dependent
    levels; `CsrSystem.precond_ordering()` returns the ordering.  See dpcg_set_precond_ic0_ordered in include/dpcg.h.
    """

    def __init__(self, mode: str = "solve", ordering: str = "caller"):
        if mode not in ("solve", "multiply"):
            raise ValueError("mode must be 'solve' or 'multiply'")
        if ordering not in ("caller", "multicolor"):
            raise ValueError("ordering must be 'caller' or 'multicolor'")
        if ordering == "multicolor" and mode != "solve":
            raise ValueError("the multicolour ordering serves the triangular solves: mode='solve'")
        self.mode = L.PRECOND_LLT_SOLVE if mode == "solve" else L.PRECOND_LLT_MULTIPLY
        self.ordering = L.ORDER_MULTICOLOR if ordering == "multicolor" else L.ORDER_CALLER

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_ic0_ordered(system._h, self.mode, self.ordering, _stream()))

    def __matmul__(self, r):
        raise TypeError("IC0 needs the system matrix: attach it with CsrSystem.set_preconditioner")


class ICholT(Preconditioner):
    """`ilupp.icholt(A, add_fill_in, threshold)` -- what the reference's harness runs by default, with `add_fill_in=1,
    threshold=0.1` (test.py:81-88) -- factored on the device the way ILU++ defines it (Saad's dual-threshold rule on the lower
    triangle): per column the candidates below threshold * ||column||_2 are dropped and of the rest the
    nnz(A[k+1:, k]) + add_fill_in largest are kept.  The ilupp binary is not available: the factor equals the restatement of
    the published algorithm (oracle/oracle.py::icholt) bit for bit, PARITY UNPINNED against ilupp's own output.
    mode="multiply" is the reference's use (it multiplies by L L^T, test.py:88), mode="solve" applies the factor by triangular
    solves.  See dpcg_set_precond_icholt in include/dpcg.h for the limits (64 kept entries per row / column), the refusals and
    the three forms of the device routine (`CsrSystem.icholt_info()` says which one ran).  Of the matrix only the entries at or
    right of the diagonal are read, in whatever order a row stores them: the factor is that of the matrix with sorted rows."""

    def __init__(self, mode: str = "multiply", add_fill_in: int = 1, threshold: float = 0.1):
        if mode not in ("solve", "multiply"):
            raise ValueError("mode must be 'solve' or 'multiply'")
        if add_fill_in < 0 or not threshold >= 0:
            raise ValueError("add_fill_in >= 0 and threshold >= 0")
        self.mode = L.PRECOND_LLT_SOLVE if mode == "solve" else L.PRECOND_LLT_MULTIPLY
        self.add_fill_in, self.threshold = int(add_fill_in), float(threshold)

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_icholt(system._h, self.mode, self.add_fill_in, self.threshold, _stream()))

    def __matmul__(self, r):
        raise TypeError("ICholT needs the system matrix: attach it with CsrSystem.set_preconditioner")


class ILUT(Preconditioner):
    """`ilupp.ilut(A)` -- the reference harness's `incomplete_lu` technique (test.py:90-93, which multiplies the factors: M = L U)
    -- factored on the device as Saad's dual-threshold ILUT(p, tau): per row, eliminated entries below threshold * ||A[i, :]||_2
    are dropped, of the rest of L's part the nnz(A[i, :i]) + add_fill_in largest stay, of U's part those >= the threshold and of
    them the nnz(A[i, i+1:]) + add_fill_in largest.  The ilupp binary is not available: the factors equal the restatement of the
    published algorithm (tests/ilut_restatement.py) bit for bit, PARITY UNPINNED against ilupp's own output.
    mode="multiply" applies z = L (U r), the reference's use; mode="solve" applies z = U^-1 (L^-1 r) by triangular solves.  M is
    not symmetric: `CsrSystem.spectrum_bounds` raises.  See dpcg_set_precond_ilut in include/dpcg.h for the limits."""

    def __init__(self, mode: str = "multiply", add_fill_in: int = 1, threshold: float = 0.1):
        if mode not in ("solve", "multiply"):
            raise ValueError("mode must be 'solve' or 'multiply'")
        if add_fill_in < 0 or not threshold >= 0:
            raise ValueError("add_fill_in >= 0 and threshold >= 0")
        self.mode = L.PRECOND_LU_SOLVE if mode == "solve" else L.PRECOND_LU_MULTIPLY
        self.add_fill_in, self.threshold = int(add_fill_in), float(threshold)

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_ilut(system._h, self.mode, self.add_fill_in, self.threshold, _stream()))

    def __matmul__(self, r):
        raise TypeError("ILUT needs the system matrix: attach it with CsrSystem.set_preconditioner")


class ILU0(Preconditioner):
    """ILU(0) of A computed at setup: the zero-fill L U factorisation for matrices whose values are not symmetric, the
    counterpart of `IC0` and the factor OpenFOAM pairs with PBiCGStab.  The factors equal the restatement
    (tests/ilu0_restatement.py) bit for bit; `CsrSystem.lu_factors()` returns them.

    variant="dilu" is OpenFOAM's DILU: only the diagonal is factored, d_i = a_ii - sum a_ik a_ki / d_k, L = I + strict_lower(A) D^-1,
    U = D + strict_upper(A); equal to ILU(0) where the pattern holds no triangle (5- / 7-point grids).

    mode="solve" applies z = U^-1 (L^-1 r) by triangular solves, mode="multiply" z = L (U r) as `ILUT`'s.

    ordering="multicolor" (solve mode): the factorisation of the matrix with its unknowns listed colour by colour -- a
    DIFFERENT preconditioner (another elimination order, more iterations) whose two triangular solves are a handful of wide
    parallel sweeps instead of hundreds of dependent levels; `CsrSystem.precond_ordering()` returns the ordering and
    `lu_factors()` the factors in it.  M is not symmetric: `CsrSystem.spectrum_bounds` raises.  See dpcg_set_precond_ilu0 in
    include/dpcg.h."""

    def __init__(self, mode: str = "solve", ordering: str = "caller", variant: str = "ilu0"):
        if mode not in ("solve", "multiply"):
            raise ValueError("mode must be 'solve' or 'multiply'")
        if ordering not in ("caller", "multicolor"):
            raise ValueError("ordering must be 'caller' or 'multicolor'")
        if variant not in ("ilu0", "dilu"):
            raise ValueError("variant must be 'ilu0' or 'dilu'")
        if ordering == "multicolor" and mode != "solve":
            raise ValueError("the multicolour ordering serves the triangular solves: mode='solve'")
        self.mode = L.PRECOND_LU_SOLVE if mode == "solve" else L.PRECOND_LU_MULTIPLY
        self.ordering = L.ORDER_MULTICOLOR if ordering == "multicolor" else L.ORDER_CALLER
        self.variant = L.ILU_DILU if variant == "dilu" else L.ILU_ILU0

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_ilu0(system._h, self.mode, self.variant, self.ordering, _stream()))

    def __matmul__(self, r):
        raise TypeError("ILU0 needs the system matrix: attach it with CsrSystem.set_preconditioner")


class FSAI(Preconditioner):
    """The factorised sparse approximate inverse (Kolotilina & Yeremin 1993): for every column i the dense SPD system
    A[P_i, P_i] y = e_1 on P_i = {j >= i : (j, i) in P} gives L[P_i, i] = y / sqrt(y_1); M = L L^T approximates A^-1 (SPD for every
    SPD A) and is only ever multiplied: z = L (L^T r), two dependency-free SpMVs.  Not in the reference -- the closed-form
    counterpart of the factor its network is trained to emit.

    level=k (1, 2 or 3): P = the structural pattern of A^k (level 1: tril(A), as IC(0)).  pattern=: tril(P) by rows as a scipy
    matrix or (rowptr, col) arrays -- lower triangular, ascending columns, the diagonal in every row; values are ignored.
    The factor equals tests/fsai_restatement.py bit for bit; `CsrSystem.factor()` returns it, `CsrSystem.fsai_info()` describes
    it.  See dpcg_set_precond_fsai in include/dpcg.h for the limits (local systems of at most 64 unknowns).  Unlike the solves, FSAI
    needs the system's rows to have strictly ascending columns: attaching it to a system created from unsorted parts raises
    DpcgError (ERR_INVALID, "ascending") and leaves the previous preconditioner in place.

    level and pattern are mutually exclusive: with a pattern, level must be left at its default (1, which then means nothing) or
    be None; any other level beside a pattern raises."""

    def __init__(self, level=1, pattern=None):
        if pattern is not None and not (level is None or (level == 1 and not isinstance(level, bool))):
            raise ValueError("level and pattern are mutually exclusive")
        if pattern is None:
            level = 1 if level is None else level
            if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 1 <= int(level) <= 3:
                raise ValueError("level must be an integer in 1..3")
            self.level, self.pattern = int(level), None
        else:
            if _is_scipy(pattern):
                P = pattern.tocsr()
                if not P.has_sorted_indices:
                    P = P.sorted_indices()
                rp, ci = P.indptr, P.indices
            else:
                try:
                    rp, ci = pattern
                except (TypeError, ValueError):
                    raise ValueError("pattern must be a scipy sparse matrix or a (rowptr, col) pair") from None
            rp = np.ascontiguousarray(rp, dtype=np.int32)
            ci = np.ascontiguousarray(ci, dtype=np.int32)
            if rp.ndim != 1 or ci.ndim != 1 or rp.size < 2 or int(rp[-1]) != ci.size or ci.size == 0:
                raise ValueError("pattern: rowptr / col do not describe a CSR pattern")
            self.level, self.pattern = None, (rp, ci)

    def _attach(self, system):
        if self.pattern is None:
            L.check(L.lib().dpcg_set_precond_fsai(system._h, self.level, _stream()))
            return
        rp, ci = self.pattern
        if rp.size != system.n + 1:
            raise ValueError("pattern size mismatch")
        L.check(L.lib().dpcg_set_precond_fsai_pattern(system._h, ci.size, _np_ptr(rp), _np_ptr(ci), L.HOST, _stream()))

    def __matmul__(self, r):
        raise TypeError("FSAI needs the system matrix: attach it with CsrSystem.set_preconditioner")


class BlockIC(Preconditioner):
    """Block-Jacobi incomplete Cholesky: the unknowns are partitioned into blocks of at most 4096 rows, every block is factored on its
    own and couplings between blocks are dropped -- OpenFOAM's DIC per subdomain of a decomposed run, PETSc's bjacobi + icc.  One
    launch applies it, one workgroup per block with the block's slice of the vector in LDS: no workgroup waits for another.  Not in
    the reference.  Between Jacobi and the global IC(0) in iterations (20^3 Poisson, 27 boxes: 46 / 22 / 15).

    blocks: an int (contiguous runs of that many rows, 1 .. 4096) or an (n,) integer array of non-negative block ids in the caller's
    numbering (any values; `poisson.subdomain_blocks` gives the boxes of a grid).  variant: "ic0" (IC(0) of the block-diagonal part)
    or "dic" (OpenFOAM's diagonal-based variant: the same on 5- / 7-point grids up to rounding, cheaper to set up, different where the
    lower triangle holds triangles).  The factor equals tests/block_ic_restatement.py bit for bit; `CsrSystem.factor()` and
    `CsrSystem.precond_ordering()` return it and its numbering, `CsrSystem.block_ic_info()` describes it.  See
    dpcg_set_precond_block_ic in include/dpcg.h for the contract, the errors and what is kept across `update_values`."""

    def __init__(self, blocks=1024, variant: str = "ic0"):
        if variant not in ("ic0", "dic"):
            raise ValueError("variant must be 'ic0' or 'dic'")
        self.variant = L.BLOCK_IC_DIC if variant == "dic" else L.BLOCK_IC_IC0
        if isinstance(blocks, (int, np.integer)) and not isinstance(blocks, bool):
            if not 1 <= int(blocks) <= 4096:
                raise ValueError("blocks must be in 1 .. 4096 rows")
            self.block_rows, self.ids = int(blocks), None
        else:
            if isinstance(blocks, torch.Tensor):
                blocks = blocks.detach().cpu().numpy()
            ids = np.asarray(blocks)
            if ids.ndim != 1 or ids.size == 0:
                raise ValueError("blocks must be an int or an (n,) integer array")
            if not np.issubdtype(ids.dtype, np.integer):
                raise ValueError("blocks must hold integers")
            if ids.size and (ids.min() < -2**31 or ids.max() > 2**31 - 1):
                raise ValueError("block ids must fit int32")
            self.block_rows, self.ids = 0, np.ascontiguousarray(ids, dtype=np.int32)

    def _attach(self, system):
        if self.ids is None:
            L.check(L.lib().dpcg_set_precond_block_ic(system._h, self.variant, self.block_rows, None, L.HOST, _stream()))
            return
        if self.ids.size != system.n:
            raise ValueError("blocks has the wrong length")
        L.check(L.lib().dpcg_set_precond_block_ic(system._h, self.variant, 0, _np_ptr(self.ids), L.HOST, _stream()))

    def __matmul__(self, r):
        raise TypeError("BlockIC needs the system matrix: attach it with CsrSystem.set_preconditioner")


class ICT(Preconditioner):
    """Thresholded incomplete Cholesky on a STATIC pattern -- tril(A) plus level-1 fill -- with MATLAB's 'ict' drop rule
    (contract: oracle/oracle.py::ict).  Not what `ilupp.icholt` computes (that is `ICholT`: a per-column entry count instead
    of a fill level); kept because a pattern known before the values lets the factorisation run level-parallel at any size.
    mode="multiply" multiplies by L L^T, mode="solve" applies the factor by triangular solves."""

    def __init__(self, mode: str = "multiply", fill_in: int = 1, threshold: float = 0.1):
        if mode not in ("solve", "multiply"):
            raise ValueError("mode must be 'solve' or 'multiply'")
        if fill_in < 0 or not threshold >= 0:
            raise ValueError("fill_in >= 0 and threshold >= 0")
        self.mode = L.PRECOND_LLT_SOLVE if mode == "solve" else L.PRECOND_LLT_MULTIPLY
        self.fill_in, self.threshold = int(fill_in), float(threshold)

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_ict(system._h, self.mode, self.fill_in, self.threshold, _stream()))

    def __matmul__(self, r):
        raise TypeError("ICT needs the system matrix: attach it with CsrSystem.set_preconditioner")


class SmoothedAggregation(Preconditioner):
    """Smoothed-aggregation algebraic multigrid applied as one V(sweeps, sweeps) cycle per update -- the reference harness's
    `algebraic_multigrid` technique (test.py:95-98: pyamg's `smoothed_aggregation_solver(A).aspreconditioner(cycle="V")`), set up
    and applied on the device (dpcg_set_precond_amg in include/dpcg.h).  The same family as pyamg's default -- symmetric strength
    with `theta`, MIS(2) aggregation, the Jacobi-smoothed prolongator with omega = (4/3) / rho(D^-1 A), Galerkin coarse operators,
    an exact solve on the coarsest level -- smoothed by damped Jacobi by default instead of pyamg's sequential Gauss-Seidel.  Parity
    with pyamg's own output is not pinned (pyamg is not a dependency); `CsrSystem.amg_hierarchy()` shows what was built.

    `smoother` picks the cycle's smoother; the hierarchy does not depend on it.  "jacobi" (the default) is damped Jacobi with
    omega = (4/3) / rho.  "gauss_seidel" is symmetric Gauss-Seidel in multicolour order: every level is coloured and one sweep
    updates colour 0, 1, .., m-1, m-2, .., 0, each colour at once.  That is the parallel counterpart of pyamg's row-by-row sweep,
    not the same operator.  A level that needs more than 63 colours keeps Jacobi, and `amg_hierarchy().smoother` says so.
    "chebyshev" is a Chebyshev polynomial of `degree` steps in D^-1 A on [rho / eig_ratio, rho].  `sweeps` counts smoother
    applications for all three; `degree` and `eig_ratio` matter for "chebyshev" only.

    `precision` is what the cycle STORES: "fp64" (the default) or "fp32".  With "fp32" the hierarchy is still built in fp64 (the
    same bits), but the values of A_l, P_l, P_l^T and dinv_l are kept a second time rounded to fp32 and every work vector of the
    cycle is fp32; all arithmetic stays fp64, PCG's r goes in and z comes out unrounded, and the dense coarse inverse stays fp64
    (dpcg_set_precond_amg_precision in include/dpcg.h has the contract).  PCG's recurrences are fp64 either way, so the accuracy a
    solve can reach does not change.  "fp32" takes "jacobi" and "chebyshev"; with "gauss_seidel" it is refused."""

    def __init__(self, theta: float = 0.0, max_levels: int = 10, max_coarse: int = 500, sweeps: int = 1, seed: int = 0,
                 smoother: str = "jacobi", degree: int = 2, eig_ratio: float = 30.0, precision: str = "fp64"):
        if not 0.0 <= float(theta) <= 1.0:
            raise ValueError("theta must lie in [0, 1]")
        if not 1 <= int(max_levels) <= 64:
            raise ValueError("max_levels must lie in 1 .. 64")
        if int(max_coarse) < 1:
            raise ValueError("max_coarse must be >= 1")
        if not 1 <= int(sweeps) <= 8:
            raise ValueError("sweeps must lie in 1 .. 8")
        if int(seed) < 0:
            raise ValueError("seed must be >= 0")
        if smoother not in AMG_SMOOTHERS:
            raise ValueError(f"smoother must be one of {', '.join(AMG_SMOOTHERS)}")
        if isinstance(degree, bool) or int(degree) != degree or not 1 <= int(degree) <= 8:
            raise ValueError("degree must be an integer in 1 .. 8")
        if not (math.isfinite(float(eig_ratio)) and float(eig_ratio) > 1.0):
            raise ValueError("eig_ratio must be finite and > 1")
        if precision not in AMG_PRECISIONS:
            raise ValueError(f"precision must be one of {', '.join(AMG_PRECISIONS)}")
        if precision == "fp32" and smoother == "gauss_seidel":
            raise ValueError("precision 'fp32' takes the smoothers 'jacobi' and 'chebyshev' (the cost of Gauss-Seidel is its colour "
                             "passes, not its bytes)")
        self.theta, self.max_levels, self.max_coarse = float(theta), int(max_levels), int(max_coarse)
        self.sweeps, self.seed = int(sweeps), int(seed)
        self.smoother, self.degree, self.eig_ratio = smoother, int(degree), float(eig_ratio)
        self.precision = precision

    def _attach(self, system):
        L.check(L.lib().dpcg_set_precond_amg_precision(system._h, self.theta, self.max_levels, self.max_coarse, self.sweeps,
                                                       self.seed & (2**64 - 1), AMG_SMOOTHERS.index(self.smoother), self.degree,
                                                       self.eig_ratio, AMG_PRECISIONS.index(self.precision), _stream()))

    def __matmul__(self, r):
        raise TypeError("SmoothedAggregation needs the system matrix: attach it with CsrSystem.set_preconditioner")


AMG_SMOOTHERS = ("jacobi", "gauss_seidel", "chebyshev")      # in the order of dpcg_amg_smoother (include/dpcg.h)
AMG_PRECISIONS = ("fp64", "fp32")                            # in the order of dpcg_amg_precision


@dataclass
class AmgLevel:
    """Level l of a hierarchy: the aggregate of each row (level 0: the caller's numbering), P_l and A_{l+1} as scipy CSR, and the
    colour of each row (int32, level 0 in the caller's numbering) when the level is smoothed by Gauss-Seidel (None otherwise)."""
    aggregates: np.ndarray
    P: "object"
    A_next: "object"
    colors: np.ndarray | None = None


@dataclass
class AmgHierarchy:
    """What `SmoothedAggregation` built (CsrSystem.amg_hierarchy): per level the rows, nnz(A_l), nnz(P_l), rho (the Lanczos estimate
    of lambda_max(D^-1 A_l)) and omega = (4/3) / rho (0 on the coarsest level, which is solved exactly); the operator and grid
    complexities; how many levels a re-attach after `update_values` took over from the previous hierarchy (0: built afresh).
    Per smoothed level (all but the coarsest): the smoother it uses ("jacobi" also where Gauss-Seidel was asked for and the level
    could not be coloured), its number of colours (0 unless Gauss-Seidel) and the Chebyshev interval (lower, upper) or None.
    `precision`: what the cycle stores, "fp64" or "fp32" (the hierarchy reported here is fp64 either way); `launches`: the kernel
    launches of one cycle.
    `level(l)` copies level l out (0 <= l < levels - 1) of the hierarchy attached NOW; it raises when that is no longer the one
    this snapshot describes (the system was re-attached meanwhile with other sizes)."""
    levels: int
    rows: list
    nnz: list
    p_nnz: list
    rho: list
    omega: list
    operator_complexity: float
    grid_complexity: float
    reused_levels: int = 0
    smoother: list = field(default_factory=list)
    colors: list = field(default_factory=list)
    chebyshev: list = field(default_factory=list)
    precision: str = "fp64"
    launches: int = 0
    _system: "object" = None

    def level(self, l: int) -> AmgLevel:
        import scipy.sparse as sp
        if not 0 <= l < self.levels - 1:
            raise IndexError("level must lie in 0 .. levels - 2")
        now = self._system.amg_hierarchy()            # the buffers are sized from the hierarchy attached now, never from a stale snapshot
        n, nc, pn, an = now.rows[l], now.rows[l + 1], now.p_nnz[l], now.nnz[l + 1]
        if (now.levels, now.rows, now.nnz, now.p_nnz) != (self.levels, self.rows, self.nnz, self.p_nnz):
            raise RuntimeError("the system's hierarchy was rebuilt since this snapshot: call amg_hierarchy() again")
        agg = np.empty(n, dtype=np.int32)
        prp, pci, pv = np.empty(n + 1, dtype=np.int32), np.empty(pn, dtype=np.int32), np.empty(pn)
        arp, aci, av = np.empty(nc + 1, dtype=np.int32), np.empty(an, dtype=np.int32), np.empty(an)
        sizes = np.array([n, pn, nc, an], dtype=np.int64)
        with torch.cuda.device(self._system.device):
            L.check(L.lib().dpcg_get_amg_level(self._system._h, int(l), _np_ptr(sizes), _np_ptr(agg), _np_ptr(prp), _np_ptr(pci),
                                               _np_ptr(pv), _np_ptr(arp), _np_ptr(aci), _np_ptr(av), _stream()))
        colors = None
        if now.smoother[l] == "gauss_seidel":
            colors = np.empty(n, dtype=np.int32)
            with torch.cuda.device(self._system.device):
                L.check(L.lib().dpcg_get_amg_colors(self._system._h, int(l), int(n), _np_ptr(colors), _stream()))
        return AmgLevel(agg, sp.csr_matrix((pv, pci, prp), shape=(n, nc)), sp.csr_matrix((av, aci, arp), shape=(nc, nc)), colors)


class _DevArray:
    """Zero-copy view of a device buffer the library hands to a callback (CUDA array interface, fp64 vector)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


class OperatorPreconditioner(Preconditioner):
    """Any object with `__matmul__` as M -- all the reference's loop asks for (`zk = M @ rk`, cg.py:61,81).

    SLOW PATH, by construction: the library calls back into Python once per update (`dpcg_set_precond_callback`),
    `op @ r` runs as whatever the object does (it receives a CUDA fp64 tensor in the caller's numbering and may
    return a CUDA or a CPU tensor / array), and the updates cannot be replayed as a hipGraph.  SpMV, dot products and
    vector updates remain the HIP kernels.  Prefer a matrix, a factor or one of the `Preconditioner` classes.
    """

    def __init__(self, op):
        if not hasattr(op, "__matmul__"):
            raise TypeError("an operator preconditioner needs __matmul__")
        self.op = op
        self.error: BaseException | None = None
        self.calls = 0

        def _apply(_user, r_ptr, z_ptr, n, _stream_ptr):
            try:
                if self.error is not None:
                    return
                dev = torch.device("cuda", torch.cuda.current_device())
                r = torch.as_tensor(_DevArray(r_ptr, n), device=dev)
                z = torch.as_tensor(_DevArray(z_ptr, n), device=dev)
                out = self.op @ r
                if isinstance(out, np.ndarray):
                    out = torch.from_numpy(out)
                z.copy_(torch.as_tensor(out).reshape(-1).to(device=dev, dtype=torch.float64))
                self.calls += 1
            except BaseException as exc:  # noqa: BLE001 - must not propagate through the C frame; re-raised after the solve
                self.error = exc

        self._fn = L.PRECOND_FN(_apply)      # kept alive with the object

    def _attach(self, system):
        self.error = None
        L.check(L.lib().dpcg_set_precond_callback(system._h, self._fn, None))

    def __matmul__(self, r):
        return self.op @ r


def as_preconditioner(M, n: int) -> Preconditioner:
    """Map whatever the reference's callers pass as `M` to an apply mode.

    None -> identity; a Preconditioner -> itself; a matrix (torch sparse/dense, scipy, numpy) ->
    Jacobi when it is exactly diagonal (bit-identical to the CSR product, one term per row),
    otherwise an explicit CSR multiply; any other object with `__matmul__` -> `OperatorPreconditioner`
    (the reference's operator protocol, honoured through a per-update callback: slow path).
    """
    if M is None:
        return Identity()
    if isinstance(M, Preconditioner):
        return M
    if isinstance(M, CsrSystem):
        raise TypeError("pass the preconditioner as a matrix or a Preconditioner, not a CsrSystem")
    try:
        space, rp, ci, v, m = csr_arrays(M)
    except TypeError:
        if hasattr(M, "__matmul__"):
            return OperatorPreconditioner(M)
        raise
    if m != n:
        raise ValueError("preconditioner size mismatch")
    if diagonal_only(rp, ci, n):
        return Jacobi(v)
    pc = CsrPreconditioner.__new__(CsrPreconditioner)
    pc.space, pc.rowptr, pc.col, pc.val, pc.n = space, rp, ci, v, m
    return pc


# --------------------------------------------------------------------------------------------
# the system operator
# --------------------------------------------------------------------------------------------
@dataclass
class SolveResult:
    x: torch.Tensor
    iterations: int
    status: int          # 0 converged, 1 max_iter, 2 breakdown
    final_res: float     # last tested <r,r>/<b,b>
    seconds: float       # wall time of the iteration loop, device-synchronised (cg.py:69,88)
    res_history: np.ndarray
    err_history: np.ndarray | None = None
    recurrence: str = "standard"   # the recurrence that RAN: "single_reduction" only when asked for and the whole-chip kernel took it


@dataclass
class RefinedSolveResult:
    """What `CsrSystem.solve_refined` returns (dpcg_solve_refined in include/dpcg.h)."""
    x: torch.Tensor
    iterations: int            # inner (fp32) updates, summed over the outer steps
    outer_steps: int           # outer residual evaluations minus one = inner solves run
    status: int                # 0 converged, 1 max_iter (cap, max_outer or stagnation), 2 breakdown
    final_res: float           # the last TRUE <r,r>/<b,b>, recomputed in fp64 = outer_history[-1]
    seconds: float             # wall time of the outer loop, device-synchronised
    res_history: np.ndarray    # iterations + 1 entries: [0] the first true value, then one rescaled recurrence value per update
    outer_history: np.ndarray  # outer_steps + 1 true values


@dataclass
class SpectrumBounds:
    """Extreme eigenvalues of M A from `CsrSystem.spectrum_bounds` (a Lanczos process on the device, dpcg_spectrum).

    kappa = lambda_max / lambda_min: the quantity that governs PCG convergence.  It equals the reference's cond(M @ A)
    (test.py:111-113, a singular-value ratio) only when M = c I.  err_min / err_max bound the distance from each Ritz value
    to an eigenvalue of M A; alpha / beta are the diagonal and off-diagonals of the Lanczos tridiagonal T_k
    (beta[k-1] = beta_{k+1}, the residual coupling)."""
    lambda_min: float
    lambda_max: float
    kappa: float
    steps: int
    converged: bool
    err_min: float
    err_max: float
    alpha: np.ndarray
    beta: np.ndarray


_REORDER_MODES = {None: L.REORDER_NONE, False: L.REORDER_NONE, "none": L.REORDER_NONE, "auto": L.REORDER_AUTO,
                  "rcm": L.REORDER_ALWAYS, True: L.REORDER_ALWAYS, "regions": L.REORDER_REGIONS}


class CsrSystem:
    """The operator A of `A @ v` (cg.py:60,75) as a CSR matrix resident in HBM.

    rowptr/col int32, val float64 or float32 CUDA tensors are borrowed (kept alive here).

    `reorder`: "auto" (default) lets the library iterate on P A P^T when the numbering scatters neighbours (large system,
    x-tile plan failed): in reverse Cuthill-McKee order when the measured x-gather traffic is > 4x the bytes used, in the
    cheap region-by-region order when only some row blocks are too scattered (OpenFOAM's numbering after refinement: BASELINE
    config 3) and the x-tile plan takes the result; "rcm" / "regions" force one, None / "none" never reorders.  Everything the caller
    passes or receives -- b, x0, x, `@`, dinv, M, L -- stays in the caller's numbering (`dpcg_reorder`, include/dpcg.h).
    """

    def __init__(self, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int, reorder="auto"):
        if not (rowptr.is_cuda and col.is_cuda and val.is_cuda):
            raise ValueError("CsrSystem expects CUDA tensors; use CsrSystem.from_host / from_any for host data")
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32:
            raise ValueError("rowptr/col must be int32")
        if val.dtype not in (torch.float64, torch.float32):
            raise ValueError("val must be float64 or float32")
        if rowptr.numel() != n + 1 or col.numel() != val.numel():
            raise ValueError("inconsistent CSR sizes")
        self._keep = (rowptr.contiguous(), col.contiguous(), val.contiguous())
        self.device = val.device
        self.n = int(n)
        self.nnz = int(col.numel())
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_create(C.byref(self._h), self.n, self.nnz, _dev_ptr(self._keep[0]),
                                        _dev_ptr(self._keep[1]), _dev_ptr(self._keep[2]),
                                        L.F64 if val.dtype == torch.float64 else L.F32, L.DEVICE, 0, _stream()))
        self._precond: Preconditioner | None = None
        self._reorder(reorder)

    def _reorder(self, mode) -> None:
        if mode not in _REORDER_MODES:
            raise ValueError("reorder must be 'auto', 'rcm', 'regions' or None")
        applied = C.c_int(0)
        if _REORDER_MODES[mode] != L.REORDER_NONE:
            with torch.cuda.device(self.device):
                L.check(L.lib().dpcg_reorder(self._h, _REORDER_MODES[mode], _stream(), C.byref(applied)))
        self.reordered = bool(applied.value)

    def update_values(self, values) -> None:
        """New matrix values on the SAME sparsity pattern (the next pressure system of one mesh), in the order of the arrays
        the system was created from.  The SpMV plan and the reordering are kept; the preconditioner is dropped -- attach one
        again.  (No reference counterpart: the reference builds a tensor per sample, test.py:61-68.)"""
        if isinstance(values, torch.Tensor) and values.is_cuda:
            v = values.detach().contiguous()
            if v.dtype not in (torch.float32, torch.float64):
                v = v.to(torch.float64)
            if v.numel() != self.nnz:
                raise ValueError(f"expected {self.nnz} values")
            if self._keep and (v.dtype != torch.float64 or v.data_ptr() % 16):
                v = v.to(torch.float64).clone()
            with torch.cuda.device(self.device):
                try:
                    L.check(L.lib().dpcg_update_values(self._h, _dev_ptr(v), L.F64 if v.dtype == torch.float64 else L.F32,
                                                       L.DEVICE, _stream()))
                except L.DpcgError:
                    self._kept_on_error = v     # (a failed null-space check comes after the handle has borrowed the new buffer)
                    raise
            if self._keep:                     # a system created from device arrays borrows them: borrow the new ones likewise --
                self._keep = (self._keep[0], self._keep[1], v)      # only once the call has succeeded (the handle still points at the old buffer otherwise)
        else:
            a = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
            dt = L.F32 if a.dtype == np.float32 else L.F64
            a = np.ascontiguousarray(a, dtype=np.float32 if dt == L.F32 else np.float64)
            if a.size != self.nnz:
                raise ValueError(f"expected {self.nnz} values")
            if self._keep:                      # borrowed device arrays: the new values must live on the device too
                return self.update_values(torch.from_numpy(a.astype(np.float64)).to(self.device))
            with torch.cuda.device(self.device):
                L.check(L.lib().dpcg_update_values(self._h, _np_ptr(a), dt, L.HOST, _stream()))
        self._precond = None

    def permutation(self):
        """perm (numpy int32, perm[new] = old) of a reordered system -- row `new` of the matrix the library iterates on is
        the caller's row `old` -- or None."""
        flag = C.c_int(0)
        perm = np.empty(self.n, dtype=np.int32)
        L.check(L.lib().dpcg_get_permutation(self._h, C.byref(flag), _np_ptr(perm), None))
        return perm if flag.value else None

    def set_nullspace(self, Z, check_tol: float = 1e-8) -> None:
        """Attach the null space of a singular (symmetric positive semi-definite) system -- a closed, all-Neumann domain -- so
        that `solve` projects it out inside PCG and returns the minimum-norm solution (dpcg_set_nullspace, include/dpcg.h).

        `Z`: "constant" (the constant vector, never stored), an array or tensor of shape (n,) or (n, k), k <= 4, with any linearly
        independent columns in the caller's numbering (orthonormalised by the library), or None to clear.  `check_tol` > 0 checks
        max|A z| <= check_tol ||A||_inf ||z||_inf for every column, now and after every `update_values`; <= 0: no check.
        Raises DpcgError (ERR_INVALID) for k > 4, a rank-deficient Z, non-finite entries and a failed check."""
        with torch.cuda.device(self.device):
            if Z is None:
                L.check(L.lib().dpcg_set_nullspace(self._h, 0, None, L.HOST, 0.0, _stream()))
                return
            if isinstance(Z, str):
                if Z != "constant":
                    raise ValueError("the only named null space is 'constant'")
                L.check(L.lib().dpcg_set_nullspace(self._h, 1, None, L.HOST, float(check_tol), _stream()))
                return
            a = Z.detach().cpu().numpy() if isinstance(Z, torch.Tensor) else np.asarray(Z)
            a = a.reshape(self.n, 1) if a.ndim == 1 and a.size == self.n else a
            if a.ndim != 2 or a.shape[0] != self.n or a.shape[1] < 1:
                raise ValueError(f"expected a null-space basis of shape ({self.n}, k)")
            cols = np.asfortranarray(a, dtype=np.float64)       # column-major n x k
            L.check(L.lib().dpcg_set_nullspace(self._h, int(cols.shape[1]), cols.ctypes.data_as(C.c_void_p), L.HOST,
                                               float(check_tol), _stream()))

    def nullspace(self):
        """The attached null space as an (n, k) numpy array with orthonormal columns in the caller's numbering, or None."""
        k = C.c_int(0)
        L.check(L.lib().dpcg_get_nullspace(self._h, C.byref(k), None))
        if k.value == 0:
            return None
        out = np.empty((self.n, k.value), dtype=np.float64, order="F")
        L.check(L.lib().dpcg_get_nullspace(self._h, C.byref(k), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_deflation(self, W, *, k: int = 8, max_steps: int = 200, rtol: float = 1e-3, seed: int = 0) -> None:
        """Attach deflation vectors, so that `solve` runs deflated PCG (dpcg_set_deflation, include/dpcg.h): the search directions
        are kept A-orthogonal to span(W), which takes the eigenvalues of M A that W captures out of the update count.

        `W`: an array or tensor of shape (n,) or (n, k), k <= 8, with any linearly independent columns in the caller's numbering (the
        library A-orthonormalises them; a dependent column is refused) -- `poisson.subdomain_indicators` gives Nicolaides'
        piecewise-constant choice without an eigen-solve; None clears; "ritz" harvests the `k` lowest Ritz vectors of M A from the
        Lanczos process of `spectrum_bounds` (dpcg_spectrum_vectors: at most `max_steps` steps, until their bounds are below
        `rtol` times the Ritz value; start vector from `seed`), evaluated against the preconditioner set at this moment.  A later
        `set_preconditioner` keeps the vectors although they were harvested for the old M: they stay valid deflation vectors, only
        no longer the low eigenvectors of the new M A.  `update_values` keeps the span and re-orthonormalises it for the new matrix.
        Raises DpcgError (ERR_INVALID) for k > 8, a dependent column, non-finite entries and a handle that has a null space."""
        self._deflation_ritz = None
        with torch.cuda.device(self.device):
            if W is None:
                L.check(L.lib().dpcg_set_deflation(self._h, 0, None, L.HOST, _stream()))
                return
            if isinstance(W, str):
                if W != "ritz":
                    raise ValueError("the only named deflation is 'ritz'")
                k = int(k)
                if not 1 <= k <= min(8, self.n):
                    raise ValueError("k must lie in 1 .. 8 and not exceed n")
                Wd = torch.empty(self.n * k, dtype=torch.float64, device=self.device)      # column-major n x k
                theta, err, steps = np.zeros(k), np.zeros(k), C.c_int(0)
                status = L.check(L.lib().dpcg_spectrum_vectors(self._h, k, int(max_steps), float(rtol), int(seed) & (2**64 - 1), _stream(),
                                                               C.byref(steps), _np_ptr(theta), _np_ptr(err), _dev_ptr(Wd)))
                if status == L.BREAKDOWN:
                    raise L.DpcgError(status, L.lib().dpcg_last_error().decode(errors="replace"))
                L.check(L.lib().dpcg_set_deflation(self._h, k, _dev_ptr(Wd), L.DEVICE, _stream()))
                self._deflation_ritz = {"theta": theta, "err": err, "steps": steps.value, "converged": status == L.OK}
                return
            a = W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else np.asarray(W)
            a = a.reshape(self.n, 1) if a.ndim == 1 and a.size == self.n else a
            if a.ndim != 2 or a.shape[0] != self.n or a.shape[1] < 1:
                raise ValueError(f"expected deflation vectors of shape ({self.n}, k)")
            cols = np.asfortranarray(a, dtype=np.float64)       # column-major n x k
            L.check(L.lib().dpcg_set_deflation(self._h, int(cols.shape[1]), cols.ctypes.data_as(C.c_void_p), L.HOST, _stream()))

    def deflation(self):
        """The attached deflation as a dict -- k, W and AW = A W as the device holds them ((n, k) numpy arrays, W^T A W = I, the
        caller's numbering) and, after set_deflation("ritz"), theta, err, steps and converged of the harvest -- or None."""
        k = C.c_int(0)
        L.check(L.lib().dpcg_get_deflation(self._h, C.byref(k), None, None))
        if k.value == 0:
            return None
        W = np.empty((self.n, k.value), dtype=np.float64, order="F")
        AW = np.empty((self.n, k.value), dtype=np.float64, order="F")
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_get_deflation(self._h, C.byref(k), _np_ptr(W), _np_ptr(AW)))
        out = {"k": k.value, "W": W, "AW": AW}
        out.update(getattr(self, "_deflation_ritz", None) or {})
        return out

    # -- constructors ----------------------------------------------------------------------
    @classmethod
    def from_host(cls, rowptr: np.ndarray, col: np.ndarray, val: np.ndarray, n: int, device=None, reorder="auto") -> "CsrSystem":
        self = cls.__new__(cls)
        self._keep = ()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.n, self.nnz = int(n), int(len(col))
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        dt = L.F32 if val.dtype == np.float32 else L.F64
        val = np.ascontiguousarray(val, dtype=np.float32 if dt == L.F32 else np.float64)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_create(C.byref(self._h), self.n, self.nnz, _np_ptr(rowptr), _np_ptr(col), _np_ptr(val),
                                        dt, L.HOST, 1, _stream()))
        self._precond = None
        self._reorder(reorder)
        return self

    @classmethod
    def from_any(cls, A, device=None, reorder="auto"):
        if isinstance(A, CsrSystem):
            return A
        space, rp, ci, v, n = csr_arrays(A)
        if space == "host":
            return cls.from_host(rp, ci, v, n, device, reorder)
        return cls(rp, ci, v, n, reorder)

    # -- bookkeeping -------------------------------------------------------------------------
    @property
    def shape(self):
        return (self.n, self.n)

    def info(self) -> dict:
        n, nnz, pn = C.c_int64(), C.c_int64(), C.c_int64()
        k, pk, ll, lu = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.check(L.lib().dpcg_get_info(self._h, C.byref(n), C.byref(nnz), C.byref(k), C.byref(pk), C.byref(pn),
                                      C.byref(ll), C.byref(lu)))
        flag, ratio = C.c_int(0), C.c_double(0.0)
        L.check(L.lib().dpcg_get_permutation(self._h, C.byref(flag), None, C.byref(ratio)))
        return {"n": n.value, "nnz": nnz.value, "spmv_kernel": ("stream", "vector", "tile")[k.value & 15],
                "two_kernel_updates": bool(k.value & 16), "spmv_nt": bool(k.value & 32), "spmv_mixed_tiles": bool(k.value & 64),
                "spmv_cyclic": bool(k.value & 128), "reordered": bool(flag.value),
                "gather_ratio": ratio.value,
                "precond": pk.value, "precond_nnz": pn.value, "levels_lower": ll.value, "levels_upper": lu.value}

    def reduction_geometry(self) -> dict:
        """How the handle's kernels sum their dot products (dpcg_get_reduction_geometry): what a checker needs to add in the same
        order (the tests' CPU restatement takes it as `device_tree=`)."""
        out = (C.c_int32 * 16)()
        L.check(L.lib().dpcg_get_reduction_geometry(self._h, out))
        return {"spmv_grid": out[0], "nrb": out[1], "cyclic": out[2], "vec_grid": out[3], "two_kernel_updates": bool(out[4]),
                "spmv_kernel": ("stream", "vector", "tile")[out[5] & 255], "spmv_tpr": out[5] >> 8, "small_threads": out[6],
                "team_eligible": bool(out[7]), "team_by_default": out[7] == 2, "rz_kind": out[8], "m_grid": out[9], "m_nrb": out[10], "m_cyclic": out[11] & 255,
                "m_tpr": (out[11] >> 8) & 255, "mt_tpr": (out[11] >> 16) & 255, "sweep_grid": out[13],
                "sweep_modes": [(out[14] >> (2 * k)) & 3 for k in range(out[12])], "sweep_paired": bool(out[15])}

    def chip_info(self) -> dict:
        """The whole-chip solve of cache-sized systems (dpcg_get_chip_info): eligibility, the geometry a checker needs to add the dot
        products in the kernel's order, and -- with DPCG_CHIP_TRACE=1 -- microseconds per update by phase of the last such solve."""
        out = (C.c_int32 * 10)()
        tr = (C.c_double * 8)()
        L.check(L.lib().dpcg_get_chip_info(self._h, out, tr))
        return {"chip_eligible": bool(out[0]), "chip_by_default": out[0] == 2, "workgroups": out[1], "threads": out[2],
                "rows_per_workgroup": out[3], "max_row_len": out[4], "max_band": out[5], "groups_on_one_xcd": bool(out[6] & 1),
                "lanes_per_row": (out[6] >> 8) & 255,
                "kernel_ms": out[7] * 1e-6,
                # the last solve, if the resident standard form ran it: (wave, slot-row) pairs that took the operands their wave holds
                # from its registers (DPCG_CHIP_SHARED=0: none), and the pairs that have a row at all
                "shared_pairs": out[8], "pairs": out[9],
                "trace_us": {"spmv": tr[0], "sum_pq": tr[1], "update_publish": tr[2], "sum_rz_rr": tr[3], "loop": tr[4],
                             "wait_pq": tr[5], "wait_rz": tr[6], "updates": int(tr[7])}}

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            L.lib().dpcg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _vec(self, v) -> torch.Tensor:
        t = _to_device_f64(v, self.device)
        if t.dim() != 1 or t.numel() != self.n:
            raise ValueError(f"expected a vector of length {self.n}")
        return t

    # -- operators -------------------------------------------------------------------------
    def __matmul__(self, v) -> torch.Tensor:
        """y = A v (cg.py:60,75)."""
        x = self._vec(v)
        y = torch.empty_like(x)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_spmv(self._h, _dev_ptr(x), _dev_ptr(y), _stream()))
        return y

    def spmv_f32(self, v: torch.Tensor) -> torch.Tensor:
        x = v.to(device=self.device, dtype=torch.float32).contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_spmv_f32(self._h, _dev_ptr(x), _dev_ptr(y), _stream()))
        return y

    def set_preconditioner(self, M) -> Preconditioner:
        pc = as_preconditioner(M, self.n)
        with torch.cuda.device(self.device):
            pc._attach(self)
        self._precond = pc
        return pc

    def precond_apply(self, r) -> torch.Tensor:
        """z = M r (cg.py:61,81) for the attached preconditioner."""
        rv = self._vec(r)
        z = torch.empty_like(rv)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_precond_apply(self._h, _dev_ptr(rv), _dev_ptr(z), _stream()))
        return z

    def sptrsv(self, rhs, upper: bool) -> torch.Tensor:
        rv = self._vec(rhs)
        out = torch.empty_like(rv)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_sptrsv(self._h, 1 if upper else 0, _dev_ptr(rv), _dev_ptr(out), _stream()))
        return out

    def precond_ordering(self):
        """(n_colors, perm) of the attached factor's own numbering: perm[k] = the caller's row at factor position k
        (identity and 0 colours unless the factor was built with ordering="multicolor")."""
        nc = C.c_int(0)
        perm = np.empty(self.n, dtype=np.int32)
        L.check(L.lib().dpcg_get_precond_ordering(self._h, C.byref(nc), _np_ptr(perm)))
        return nc.value, perm

    def factor(self):
        """The attached L factor as host CSR arrays (rowptr, col, val), in the factor's numbering (`precond_ordering`)."""
        nnz = self.info()["precond_nnz"]
        rp = np.empty(self.n + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        v = np.empty(nnz, dtype=np.float64)
        L.check(L.lib().dpcg_get_factor(self._h, _np_ptr(rp), _np_ptr(ci), _np_ptr(v)))
        return rp, ci, v

    def fsai_info(self) -> dict:
        """The attached `FSAI` factor (dpcg_get_fsai_info): level (0: explicit pattern), the largest local system, the columns per
        width class of the device kernels, whether the last attach reused the symbolic phase.  DpcgError (ERR_STATE) otherwise."""
        out = (C.c_int32 * 8)()
        L.check(L.lib().dpcg_get_fsai_info(self._h, out))
        return {"level": out[0], "max_m": out[1], "columns_by_width": {w: out[2 + k] for k, w in enumerate((4, 8, 16, 32, 64))},
                "pattern_reused": bool(out[7])}

    def block_ic_info(self) -> dict:
        """The attached `BlockIC` factor (dpcg_get_block_ic_info): variant, number of blocks, rows of the largest block, the most
        dependency levels of L and of L^T in any block (the barriers of an apply), the apply kernel's workgroup size, whether the last
        attach reused the symbolic phase.  DpcgError (ERR_STATE) otherwise."""
        out = (C.c_int32 * 8)()
        L.check(L.lib().dpcg_get_block_ic_info(self._h, out))
        return {"variant": ("ic0", "dic")[out[0]], "blocks": out[1], "max_block": out[2], "levels_lower": out[3], "levels_upper": out[4],
                "threads": out[5], "pattern_reused": bool(out[6])}

    def icholt_info(self) -> dict:
        """How the attached `ICholT` factor was produced (dpcg_get_icholt_info): `form` (1 the LDS pipeline, 2 the workspace pipeline,
        3 one wave), `waves` of that pipeline (0 for form 3), `retry_column` (the column at which a pipeline attempt stopped and
        form 3 factored the matrix again; None when no pipeline ran or it finished) and `pool_cap`, the pool bound the dispatcher
        compared with its limits.  DpcgError (ERR_STATE) when the attached preconditioner is not an `ICholT` factor."""
        out = (C.c_int32 * 4)()
        L.check(L.lib().dpcg_get_icholt_info(self._h, out))
        return {"form": out[0], "waves": out[1], "retry_column": None if out[2] < 0 else out[2], "pool_cap": out[3]}

    def lu_factors(self):
        """The attached `ILUT` / `ILU0` factors (L, U) as scipy CSR in the factor's numbering (`precond_ordering`: the caller's
        unless built with ordering="multicolor"): L unit lower (diagonal last), U upper (diagonal first).  DpcgError (ERR_STATE)
        when no L U factor is attached."""
        import scipy.sparse as sp
        ln, un = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().dpcg_get_lu_factors(self._h, C.byref(ln), C.byref(un), None, None, None, None, None, None))
        out = []
        for nnz in (ln.value, un.value):
            out.append((np.empty(self.n + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32), np.empty(nnz, dtype=np.float64)))
        (lr, lc, lv), (ur, uc, uv) = out
        L.check(L.lib().dpcg_get_lu_factors(self._h, None, None, _np_ptr(lr), _np_ptr(lc), _np_ptr(lv), _np_ptr(ur), _np_ptr(uc),
                                            _np_ptr(uv)))
        return (sp.csr_matrix((lv, lc, lr), shape=(self.n, self.n)), sp.csr_matrix((uv, uc, ur), shape=(self.n, self.n)))

    def spmv_dot_bench(self, repeats: int = 100) -> float:
        """Average milliseconds of the in-PCG SpMV+<p,Ap> kernel over `repeats` launches (HIP events)."""
        x = torch.rand(self.n, device=self.device, dtype=torch.float64)
        y = torch.empty_like(x)
        ms = C.c_float()
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_spmv_dot_bench(self._h, _dev_ptr(x), _dev_ptr(y), repeats, C.byref(ms), _stream()))
        return float(ms.value)

    def solve(self, b, x0=None, *, rtol_sq: float = 1e-8, atol_sq: float = 0.0, max_iter: int = 1024, flags: int = 0,
              x_true=None, want_history: bool = True, guess: "ProjectedGuess | None" = None,
              recurrence: str = "standard") -> SolveResult:
        """Run the PCG loop of cg.py:58-90 on the GPU (see dpcg_solve in include/dpcg.h).

        `recurrence="single_reduction"` (DPCG_SINGLE_REDUCTION): Chronopoulos and Gear's form of CG in the whole-chip kernel -- one
        chip-wide exchange an update instead of two, other bits than the reference's recurrence.  M = I or Jacobi, fp64, systems the
        resident whole-chip form takes; anything else raises DpcgError (ERR_INVALID) with the reason.  `SolveResult.recurrence` names
        the recurrence that ran ("standard" when the kernel could not become co-resident and the launches took over).

        `guess` (a `ProjectedGuess` of this system): the solve starts from the projection of b onto the span of the earlier
        solutions and hands its own solution to the guess afterwards (a capped solve too; a breakdown does not).  Not together
        with `x0`."""
        if recurrence not in L.RECURRENCES:
            raise ValueError(f"recurrence must be one of {L.RECURRENCES}, not {recurrence!r}")
        if recurrence == "single_reduction":
            flags = int(flags) | L.SINGLE_REDUCTION
        bv = self._vec(b)
        if guess is not None:
            if x0 is not None:
                raise ValueError("pass either x0 or guess, not both")
            if guess.system is not self:
                raise ValueError("the guess belongs to another system")
            x0 = guess.project(bv)
        x0v = None if x0 is None else self._vec(x0)
        xt = None if x_true is None else self._vec(x_true)
        x = torch.empty_like(bv)
        hist = np.full(max_iter + 1, np.nan) if want_history else None
        err = np.full(max_iter + 1, np.nan) if xt is not None else None
        iters, res, sec = C.c_int(), C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            status = L.check(L.lib().dpcg_solve(
                self._h, _dev_ptr(bv), _dev_ptr(x0v), _dev_ptr(x), rtol_sq, atol_sq, int(max_iter), int(flags),
                _stream(), C.byref(iters), C.byref(res), C.byref(sec), _np_ptr(hist), _dev_ptr(xt), _np_ptr(err)))
        if isinstance(self._precond, OperatorPreconditioner) and self._precond.error is not None:
            err, self._precond.error = self._precond.error, None
            raise err
        k = iters.value
        if guess is not None and status != L.BREAKDOWN:
            guess.update(x)
        ran = C.c_int(0)
        L.check(L.lib().dpcg_get_last_recurrence(self._h, C.byref(ran)))
        return SolveResult(x, k, status, res.value, sec.value, hist[: k + 1] if hist is not None else np.empty(0),
                           err[: k + 1] if err is not None else None, L.RECURRENCES[ran.value])

    def solve_refined(self, b, x0=None, *, rtol_sq: float = 1e-8, atol_sq: float = 0.0, max_iter: int = 1024,
                      inner_rtol_sq: float = 1e-6, max_outer: int = 16, want_history: bool = True) -> RefinedSolveResult:
        """Mixed-precision PCG (dpcg_solve_refined in include/dpcg.h): inner PCG updates whose matrix values and vectors are stored
        in fp32, inside an fp64 loop that recomputes the true residual and corrects x.  Opt-in; M = I or Jacobi only, no null space
        and no deflation -- anything else raises DpcgError (ERR_INVALID) with the reason.  `final_res` is a true residual."""
        bv = self._vec(b)
        x0v = None if x0 is None else self._vec(x0)
        x = torch.empty_like(bv)
        hist = np.full(max(int(max_iter), 0) + 1, np.nan) if want_history else None
        outer_hist = np.full(max(int(max_outer), 0) + 1, np.nan)
        iters, outer, res, sec = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            status = L.check(L.lib().dpcg_solve_refined(
                self._h, _dev_ptr(bv), _dev_ptr(x0v), _dev_ptr(x), rtol_sq, atol_sq, int(max_iter), float(inner_rtol_sq),
                int(max_outer), 0, _stream(), C.byref(iters), C.byref(outer), C.byref(res), C.byref(sec), _np_ptr(hist),
                _np_ptr(outer_hist)))
        k = iters.value
        return RefinedSolveResult(x, k, outer.value, status, res.value, sec.value,
                                  hist[: k + 1] if hist is not None else np.empty(0), outer_hist[: outer.value + 1])

    def solve_bicgstab(self, b, x0=None, *, rtol_sq: float = 1e-8, atol_sq: float = 0.0, max_iter: int = 1024,
                       graph: bool = True) -> SolveResult:
        """Right-preconditioned BiCGStab (dpcg_solve_bicgstab in include/dpcg.h) for a system whose values are not symmetric, or
        whose preconditioner is not (`ILUT`, an explicit `CsrPreconditioner`).  Every preconditioner but an `OperatorPreconditioner`
        is taken; a handle with a null space or a deflation raises DpcgError (ERR_INVALID) with the reason.  `res_history[k]` is
        <r_k,r_k>/<b,b> of the original system, `status` 0 converged / 1 max_iter / 2 breakdown; `recurrence` says "bicgstab".
        `graph=False` passes DPCG_NO_GRAPH (accepted: this driver replays no graph, the bits are the same)."""
        bv = self._vec(b)
        x0v = None if x0 is None else self._vec(x0)
        x = torch.empty_like(bv)
        hist = np.full(max(int(max_iter), 0) + 1, np.nan)
        iters, res, sec = C.c_int(), C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            status = L.check(L.lib().dpcg_solve_bicgstab(
                self._h, _dev_ptr(bv), _dev_ptr(x0v), _dev_ptr(x), rtol_sq, atol_sq, int(max_iter), 0 if graph else L.NO_GRAPH,
                _stream(), C.byref(iters), C.byref(res), C.byref(sec), _np_ptr(hist)))
        k = iters.value
        return SolveResult(x, k, status, res.value, sec.value, hist[: k + 1], None, "bicgstab")

    def amg_hierarchy(self) -> AmgHierarchy:
        """The smoothed-aggregation hierarchy of the attached `SmoothedAggregation` preconditioner (DpcgError otherwise)."""
        cap = 64
        nl = C.c_int(0)
        rows, nnz, pnnz = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
        rho, omega = np.zeros(cap), np.zeros(cap)
        oc, gc, reused = C.c_double(), C.c_double(), C.c_int(0)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_get_amg_info(self._h, cap, C.byref(nl), _np_ptr(rows), _np_ptr(nnz), _np_ptr(pnnz), _np_ptr(rho),
                                              _np_ptr(omega), C.byref(oc), C.byref(gc), C.byref(reused)))
        k = nl.value
        sm, ncol, lo, hi = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap)
        with torch.cuda.device(self.device):
            L.check(L.lib().dpcg_get_amg_smoothers(self._h, cap, _np_ptr(sm), _np_ptr(ncol), _np_ptr(lo), _np_ptr(hi)))
            prec = C.c_int(0)
            L.check(L.lib().dpcg_get_amg_precision(self._h, C.byref(prec)))
            launches = C.c_int(0)
            L.check(L.lib().dpcg_get_amg_launches(self._h, C.byref(launches), None))
        m = max(k - 1, 0)
        cheb = [(float(a), float(b)) if int(t) == L.AMG_CHEBYSHEV else None for t, a, b in zip(sm[:m], lo[:m], hi[:m])]
        return AmgHierarchy(k, [int(v) for v in rows[:k]], [int(v) for v in nnz[:k]], [int(v) for v in pnnz[:k]],
                            [float(v) for v in rho[:k]], [float(v) for v in omega[:k]], oc.value, gc.value, reused.value,
                            smoother=[AMG_SMOOTHERS[int(v)] for v in sm[:m]], colors=[int(v) for v in ncol[:m]], chebyshev=cheb,
                            precision=AMG_PRECISIONS[prec.value], launches=launches.value, _system=self)

    def spectrum_bounds(self, *, max_steps: int = 1000, rtol: float = 1e-6, seed: int = 0) -> SpectrumBounds:
        """Extreme eigenvalues of M A for the attached preconditioner M (M = I without one) and kappa = lambda_max / lambda_min,
        at any size (dpcg_spectrum: Lanczos in the M inner product, fully reorthogonalised, basis resident on the device;
        test.py:111-113 forms M A densely instead).  M must be symmetric positive definite: when the process finds it is not,
        this raises DpcgError (status 2) instead of returning a number.  An OperatorPreconditioner works (one host call per
        step: slow) -- keeping it symmetric positive definite is the caller's promise.  The result does not depend on the
        handle's numbering; the same seed gives the same bits.  Memory: 2 x (min(max_steps, n) + 1) x n doubles."""
        m = max(1, min(int(max_steps), self.n))
        alpha = np.zeros(m)
        beta = np.zeros(m)
        k = C.c_int(0)
        tmin, tmax, emin, emax = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        with torch.cuda.device(self.device):
            status = L.check(L.lib().dpcg_spectrum(self._h, int(max_steps), float(rtol), int(seed) & (2**64 - 1), _stream(),
                                                   C.byref(k), C.byref(tmin), C.byref(tmax), C.byref(emin), C.byref(emax),
                                                   _np_ptr(alpha), _np_ptr(beta)))
        if isinstance(self._precond, OperatorPreconditioner) and self._precond.error is not None:
            err, self._precond.error = self._precond.error, None
            raise err
        if status == L.BREAKDOWN:
            raise L.DpcgError(status, L.lib().dpcg_last_error().decode(errors="replace"))
        steps = k.value
        kappa = tmax.value / tmin.value if tmin.value > 0 else float("nan")
        return SpectrumBounds(tmin.value, tmax.value, kappa, steps, status == L.OK, emin.value, emax.value,
                              alpha[:steps].copy(), beta[:steps].copy())


class ProjectedGuess:
    """Initial guesses for a SEQUENCE of solves on one system, projected from the solutions so far (dpcg_guess_*, include/dpcg.h;
    P. F. Fischer, CMAME 163, 1998): `system.solve(b, guess=guess)` starts from the A-norm-best approximation of the solution in
    the span of up to `depth` earlier ones.  The basis lives on the device in the caller's numbering; `update_values` is noticed
    (the basis is re-orthonormalised against the new matrix before its next use).  No reference counterpart (cg.py:58 starts
    from zeros)."""

    def __init__(self, system: "CsrSystem", depth: int = 8, tol_dep: float = 1e-7):
        self.system = system
        self.depth = int(depth)
        self._g = C.c_void_p()
        with torch.cuda.device(system.device):
            L.check(L.lib().dpcg_guess_create(system._h, int(depth), float(tol_dep), C.byref(self._g)))

    def project(self, b) -> torch.Tensor:
        """x0 = X~ (X~^T b); zeros while the basis is empty.  Raises DpcgError (ERR_INVALID) when b holds a non-finite value."""
        bv = self.system._vec(b)
        x0 = torch.empty_like(bv)
        with torch.cuda.device(self.system.device):
            L.check(L.lib().dpcg_guess_project(self._g, _dev_ptr(bv), _dev_ptr(x0), _stream()))
        return x0

    def update(self, x) -> None:
        """Hand the solution of the system last projected for to the basis (appended, skipped as dependent, or a restart)."""
        xv = self.system._vec(x)
        with torch.cuda.device(self.system.device):
            L.check(L.lib().dpcg_guess_update(self._g, _dev_ptr(xv), _stream()))

    def reset(self) -> None:
        L.check(L.lib().dpcg_guess_reset(self._g))

    def info(self) -> dict:
        out = (C.c_int32 * 8)()
        L.check(L.lib().dpcg_guess_info(self._g, out))
        return {"depth": out[0], "size": out[1], "restarts": out[2], "appended": out[3], "skipped": out[4], "dropped": out[5],
                "reorthonormalisations": out[6], "values_epoch": out[7]}

    def basis(self):
        """(X~, W) as host arrays of shape (n, size), W = A X~ (for tests)."""
        size = self.info()["size"]
        X = np.zeros((self.system.n, size), order="F")
        W = np.zeros((self.system.n, size), order="F")
        with torch.cuda.device(self.system.device):
            L.check(L.lib().dpcg_guess_get_basis(self._g, _np_ptr(X), _np_ptr(W)))
        return X, W

    def close(self) -> None:
        if getattr(self, "_g", None) is not None and self._g.value:
            L.lib().dpcg_guess_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def tridiag_ritz(alpha, beta):
    """(theta, bottom) of the symmetric tridiagonal tridiag(beta, alpha, beta): eigenvalues ascending and the last component of
    each unit eigenvector (host only, dpcg_tridiag_ritz: implicit QL)."""
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta, dtype=np.float64)
    k = a.size
    if b.size < k - 1:
        raise ValueError("beta needs len(alpha) - 1 entries")
    theta = np.empty(k)
    bottom = np.empty(k)
    L.check(L.lib().dpcg_tridiag_ritz(k, _np_ptr(a), _np_ptr(b) if k > 1 else None, _np_ptr(theta), _np_ptr(bottom)))
    return theta, bottom


def tridiag_eigvecs(alpha, beta, k):
    """(theta, S): the k lowest eigenvalues of tridiag(beta, alpha, beta), ascending, and their unit eigenvectors as the columns of
    S, shape (len(alpha), k), signs arbitrary (host only, dpcg_tridiag_eigvecs: implicit QL with accumulated rotations)."""
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta, dtype=np.float64)
    m = a.size
    if b.size < m - 1:
        raise ValueError("beta needs len(alpha) - 1 entries")
    if not 1 <= int(k) <= m:
        raise ValueError("k must lie in 1 .. len(alpha)")
    theta = np.empty(int(k))
    S = np.empty((m, int(k)), order="F")
    L.check(L.lib().dpcg_tridiag_eigvecs(m, _np_ptr(a), _np_ptr(b) if m > 1 else None, int(k), _np_ptr(theta), _np_ptr(S)))
    return theta, S


def dot(a: torch.Tensor, b: torch.Tensor) -> float:
    """<a,b> by the deterministic two-stage HIP reduction (torch.inner at cg.py:17,76,78,82)."""
    a = a.to(torch.float64).contiguous()
    b = b.to(device=a.device, dtype=torch.float64).contiguous()
    out = C.c_double()
    with torch.cuda.device(a.device):
        L.check(L.lib().dpcg_dot(a.numel(), _dev_ptr(a), _dev_ptr(b), C.byref(out), _stream()))
    return float(out.value)


def stream_bench(n_read: int = 2, write: bool = True, out_bytes: int = 1 << 27, repeats: int = 10, nontemporal: bool = False,
                 walk: bool = False) -> float:
    """GB/s (reads + writes) of the library's own streaming kernel on this box: per 16 bytes written, `n_read` x 16
    contiguous bytes are read (or only reduced when write=False) -- the measured HBM ceiling next to the 8 TB/s spec
    (SURVEY.md 8-d2).  n_read = 11 with write is the read:write ratio of a 7-point CSR SpMV."""
    ms, moved = C.c_float(), C.c_int64()
    # walk: the streams walked together by the whole grid instead of one slab per workgroup (a copy then is the guide's
    # float4-copy shape: one 16-byte element per thread)
    L.check(L.lib().dpcg_stream_bench(int(n_read), 1 if write else 0, (1 if nontemporal else 0) | (2 if walk else 0), int(out_bytes), int(repeats),
                                      C.byref(ms), C.byref(moved), _stream()))
    return moved.value / (ms.value * 1e-3) / 1e9


def release_cached_memory() -> None:
    """Return the device blocks the library keeps between setups (see include/dpcg.h) to the driver."""
    L.check(L.lib().dpcg_release_cached_memory())
