"""The FSAI edge cases shared by tests/test_fsai_edges_host.py (CPU) and tests/test_fsai_edges_gpu.py: small systems from
tests/edge_matrices.py chosen so that every width class of the device kernels (m <= 4, 8, 16, 32, 64; dpcg_fsai.hip) is entered on
both sides of its boundaries, at the cap m = 64, with padded and partly filled waves, with values of both signs, scaled over many
decades, with stored zeros, and the inputs the routine is written to refuse.

A `Case` names the matrix, how the factor is attached (a level, or an explicit lower pattern) and the width facts the host test
re-asserts with tests/fsai_restatement.py: the columns per class, the widest local system and the widths that occur exactly
`count` times (`hits`).  An `ErrorCase` names what the restatement raises; the device must raise the same.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import scipy.sparse as sp

import edge_matrices as E

BOUNDARY_WIDTHS = (1, 4, 5, 8, 9, 16, 17, 32, 33)      # both sides of every class boundary: once each in the banded cases


@dataclass(frozen=True)
class Case:
    name: str
    matrix: Callable[[], sp.csr_matrix]
    level: Optional[int]                                # 1 .. 3, or None with `pattern`
    counts: tuple                                       # columns with m <= 4, 5 .. 8, 9 .. 16, 17 .. 32, 33 .. 64
    max_m: int
    pattern: Optional[Callable[[], sp.csr_matrix]] = None
    hits: dict = field(default_factory=dict)            # width -> the number of columns that have exactly this width
    all_widths_to: int = 0                              # every width 1 .. all_widths_to occurs


@dataclass(frozen=True)
class ErrorCase:
    name: str
    matrix: Callable[[], sp.csr_matrix]
    level: int
    kind: str                                           # "width" or "pivot"
    column: int
    m: int = 0                                          # width errors: the m of that column


def diags_1_to_130() -> sp.csr_matrix:
    """A diagonal matrix: every m = 1, four of the five classes are empty."""
    return E.csr(sp.diags(np.arange(1.0, 131.0)))


def band40_pattern() -> sp.csr_matrix:
    """tril of a full band of half-bandwidth 40 on 256 rows: far wider than the 5-point grid it is attached to."""
    return sp.tril(E.banded_spd(256, 40)).tocsr()


def _once(widths=BOUNDARY_WIDTHS):
    return {w: 1 for w in widths}


CASES = (
    Case("banded200_63", lambda: E.banded_spd(200, 63), 1, (4, 4, 8, 16, 168), 64, hits={**_once(), 64: 137}, all_widths_to=64),
    Case("banded150_21_l3", lambda: E.banded_spd(150, 21), 3, (4, 4, 8, 16, 118), 64, hits={**_once(), 64: 87}, all_widths_to=64),
    Case("banded200_63_scaled8", lambda: E.scaled_rows(E.banded_spd(200, 63)), 1, (4, 4, 8, 16, 168), 64,
         hits={**_once(), 64: 137}, all_widths_to=64),
    Case("banded200_63_scaled70", lambda: E.scaled_rows(E.banded_spd(200, 63), -70, 70), 1, (4, 4, 8, 16, 168), 64,
         hits={**_once(), 64: 137}, all_widths_to=64),
    Case("random_bbt600", lambda: E.random_bbt(600), 1, (256, 227, 116, 1, 0), 17, hits={17: 1}),
    Case("stored_zeros_poisson20", lambda: E.with_stored_zeros(E.poisson2d(20)), 2, (18, 30, 352, 0, 0), 14),
    Case("jumping24_b4", lambda: E.jumping((24, 24), 4), 2, (47, 529, 0, 0, 0), 7),
    Case("anisotropic24", lambda: E.anisotropic2d(24, 1e-6), 3, (25, 26, 525, 0, 0), 13),
    Case("tiny_components", E.tiny_components, 2, (50, 529, 0, 0, 0), 7),
    Case("boundary_identity20", lambda: E.boundary_identity(20), 2, (60, 340, 0, 0, 0), 7),
    Case("tiny1", lambda: E.tiny(1), 3, (1, 0, 0, 0, 0), 1),
    Case("tiny2", lambda: E.tiny(2), 3, (2, 0, 0, 0, 0), 2),
    Case("tiny3", lambda: E.tiny(3), 3, (3, 0, 0, 0, 0), 3),
    Case("diags130", diags_1_to_130, 2, (130, 0, 0, 0, 0), 1, hits={1: 130}),
    Case("poisson16_band40_pattern", lambda: E.poisson2d(16), None, (4, 4, 8, 16, 224), 41, pattern=band40_pattern,
         hits={**_once(), 41: 216}, all_widths_to=41),
)
# level 1 at the smallest shapes the transposes of the symbolic phase see: one row; every column of the strictly lower part empty
DEGENERATE_CASES = (
    Case("tiny1_l1", lambda: E.tiny(1), 1, (1, 0, 0, 0, 0), 1, hits={1: 1}),
    Case("diags5_l1", lambda: E.csr(sp.diags(np.arange(1.0, 6.0))), 1, (5, 0, 0, 0, 0), 1, hits={1: 5}),
)
CASE_BY_NAME = {c.name: c for c in CASES + DEGENERATE_CASES}


def _with(A, entries) -> sp.csr_matrix:
    """A with the given (row, col) -> value entries overwritten (all of them stored already)."""
    A = A.copy()
    for (r, c), v in entries.items():
        k = A.indptr[r] + int(np.searchsorted(A.indices[A.indptr[r]:A.indptr[r + 1]], c))
        assert A.indices[k] == c
        A.data[k] = v
    return A


def _with_data(A, k, v) -> sp.csr_matrix:
    A = A.copy()
    A.data[k] = v
    return A


def _inf_entry_index() -> int:
    return int(E.banded_spd(200, 20).indptr[100]) + 3


def reg_and_wide_both_fail() -> sp.csr_matrix:
    """tiny(3) with a negative last diagonal entry (columns 0 .. 2: the class m <= 4) in front of banded_spd(100, 20) with a negative
    diagonal entry at its row 50 (columns 3 ..: the class m <= 32 fails too).  The lowest failing column is in the register class."""
    T = _with(E.tiny(3), {(2, 2): -1.0})
    B = _with(E.banded_spd(100, 20), {(50, 50): -1.0})
    return E.csr(sp.block_diag([T, B]))


ERROR_CASES = (
    ErrorCase("banded200_64", lambda: E.banded_spd(200, 64), 1, "width", 0, 65),
    ErrorCase("banded150_22_l3", lambda: E.banded_spd(150, 22), 3, "width", 0, 67),
    ErrorCase("random_bbt600_l2", lambda: E.random_bbt(600), 2, "width", 1, 72),
    ErrorCase("banded200_63_neg150", lambda: _with(E.banded_spd(200, 63), {(150, 150): -1.0}), 1, "pivot", 87),
    ErrorCase("banded200_20_neg30_neg170", lambda: _with(E.banded_spd(200, 20), {(30, 30): -1.0, (170, 170): -1.0}), 1, "pivot", 10),
    ErrorCase("banded200_20_inf", lambda: _with_data(E.banded_spd(200, 20), _inf_entry_index(), np.inf), 1, "pivot", 80),
    ErrorCase("banded200_20_nan", lambda: _with_data(E.banded_spd(200, 20), _inf_entry_index(), np.nan), 1, "pivot", 80),
    # the lowest failing column is 1 (P_1 = {1, 2} holds row 2; P_0 = {0, 1} does not), solved by k_fsai_reg<4>; columns 33 .. 53
    # fail in k_fsai_wide<32>
    ErrorCase("reg_and_wide_both_fail", reg_and_wide_both_fail, 1, "pivot", 1),
    # every Cholesky pivot is positive and finite, but y_0 ~ 1 / a_ii overflows: only the test of y_0 refuses these (the values are
    # subnormal; m = 1 in k_fsai_reg<4>, m = 21 in k_fsai_wide<32>)
    ErrorCase("y0_overflows_reg", lambda: _with(diags_1_to_130(), {(5, 5): 1e-320}), 2, "pivot", 5),
    ErrorCase("y0_overflows_wide", lambda: E.csr(E.banded_spd(200, 20) * 1e-311), 1, "pivot", 0),
)
ERROR_CASE_BY_NAME = {c.name: c for c in ERROR_CASES}


def reversed_rows(A):
    """(rowptr, col, val) of A with the entries of every row in descending column order."""
    A = E.csr(A)
    rp = A.indptr.astype(np.int32)
    ci, v = A.indices.astype(np.int32).copy(), A.data.copy()
    for i in range(A.shape[0]):
        s, e = rp[i], rp[i + 1]
        ci[s:e], v[s:e] = ci[s:e][::-1].copy(), v[s:e][::-1].copy()
    return rp, ci, v


def first_two_swapped(A):
    """(rowptr, col, val) of A with the first two entries exchanged in every row that holds two or more entries left of its diagonal:
    the diagonal and the upper part stay where a bisection finds them, the two lower entries do not."""
    A = E.csr(A)
    rp = A.indptr.astype(np.int32)
    ci, v = A.indices.astype(np.int32).copy(), A.data.copy()
    for i in range(A.shape[0]):
        s = rp[i]
        if rp[i + 1] - s > 2 and ci[s + 1] < i:
            ci[s], ci[s + 1] = ci[s + 1], ci[s]
            v[s], v[s + 1] = v[s + 1], v[s]
    return rp, ci, v
