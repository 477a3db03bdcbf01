"""The ICholT edge cases shared by tests/test_icholt_edges_host.py (CPU) and tests/test_icholt_edges_gpu.py: small systems chosen
so that every form of the device routine (dpcg_icholt.hip: the LDS pipeline, the workspace pipeline, the one-wave kernel) is entered
on both sides of the dispatcher's limits, every cap is met exactly and exceeded by one, the selection meets ties, a candidate on
the threshold, exact zeros and values at the ends of the fp64 range, and the input is stored in ways a caller may store it.

A `Case` names the matrix, the arguments, the environment it runs under and what is expected: a factor (`refusal` is None), or a
refusal kind (oracle.IcholtError.kind) with its column; which form must report the factor and whether the pipeline may hand the
matrix to the one-wave kernel (`retry`: None, or the column).  The facts a case is built for (`facts`) are re-asserted on the CPU
with oracle.icholt's `stats`.

The dispatcher's limits are stated ONCE, here (`predict`), as include/dpcg.h documents them.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import scipy.sparse as sp

import edge_matrices as E

# ---- the dispatcher (icholt_factor) -----------------------------------------------------------------------------------------
LDS_MAX_ROWS = 4096                 # 12-bit row and column fields
WORKSPACE_MAX_ROWS = 8192           # 13-bit fields
LDS_BYTES = 160 * 1024
POOL_LIMIT = 0xff00
CAP = 64                            # kept entries per row and per column of L, candidates the pipeline holds
CAND_CAP = 256


def pool_cap(n: int, nnz: int, add_fill_in: int) -> int:
    return (nnz - n + 1) // 2 + n * add_fill_in + 1


def lds_bytes(n: int, cap: int, waves: int) -> int:
    pool, rows = cap + 64, (n + 3) & ~3
    return 4096 + 256 * (waves + 8) + 14 * pool + 2 * (pool & 1) + 18 * rows


def predict(rp, ci, add_fill_in: int, env: dict) -> tuple:
    """(form, waves, retry column or None, pool_cap) as dpcg_get_icholt_info must report them for a matrix every form accepts: 1 the
    LDS pipeline, 2 the workspace pipeline, 3 the one-wave kernel.  The one retry this predicts is the staging's: the columns of A
    the pipeline stages (the entries right of the diagonal, plus add_fill_in each) do not fit the pool bound, which is computed
    from nnz as if the pattern were symmetric."""
    n, nnz = len(rp) - 1, int(rp[-1])
    lds = env.get("DPCG_ICHOLT_LDS", "1")
    waves = int(env.get("DPCG_ICHOLT_WAVES", "4"))
    cap = pool_cap(n, nnz, add_fill_in)
    in_lds = n <= LDS_MAX_ROWS and lds_bytes(n, cap, waves) + 64 <= LDS_BYTES and lds != "2"
    in_mem = not in_lds and n <= WORKSPACE_MAX_ROWS
    if lds == "0" or cap >= POOL_LIMIT or not (in_lds or in_mem):
        return 3, 0, None, cap
    upper = int(np.count_nonzero(np.asarray(ci) > np.repeat(np.arange(n), np.diff(rp))))
    if upper + n * add_fill_in > cap:
        return 3, 0, 0, cap
    return (1, waves, None, cap) if in_lds else (2, 8 if waves == 8 else 4, None, cap)


@dataclass(frozen=True)
class Case:
    name: str
    matrix: Callable[[], object]                         # a scipy CSR, or (rowptr, col, val) where the storage itself is the case
    add_fill_in: int
    threshold: float
    env: dict = field(default_factory=dict)
    refusal: Optional[str] = None                        # None: a factor; else "colcap" | "cand" | "rowcap" | "pivot" | "nodiag"
    column: Optional[int] = None                         # the column a refusal names
    form: Optional[int] = None                           # the form that must report the factor (None: whatever `predict` says)
    retry: Optional[int] = None                          # the column at which the pipeline must hand over (None: it must not)
    nonfinite: bool = False                              # the factor holds inf: compared by bits, not applied
    facts: dict = field(default_factory=dict)            # what the host test re-asserts (see test_icholt_edges_host.py)


def arrays(M):
    """(rowptr, col, val) of a case's matrix as the device is given it."""
    if isinstance(M, tuple):
        return M
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def as_csr(M) -> sp.csr_matrix:
    """The matrix a case's storage means (rows as stored; oracle.icholt sorts a copy)."""
    if isinstance(M, tuple):
        rp, ci, v = M
        return sp.csr_matrix((v.copy(), ci.copy(), rp.copy()), shape=(len(rp) - 1, len(rp) - 1))
    return M


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _spd(n, rows, cols, vals, diag=None) -> sp.csr_matrix:
    """The symmetric matrix with the given strict-upper entries mirrored and a strictly dominant diagonal (sum |row| + 1) unless
    `diag` gives one; stored zeros are kept."""
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    assert (rows < cols).all()
    dom = np.bincount(rows, np.abs(vals), n) + np.bincount(cols, np.abs(vals), n) + 1.0
    d = dom if diag is None else np.asarray(diag, dtype=np.float64)
    r = np.concatenate([rows, cols, np.arange(n)])
    c = np.concatenate([cols, rows, np.arange(n)])
    v = np.concatenate([vals, vals, d])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    assert not ((r[1:] == r[:-1]) & (c[1:] == c[:-1])).any()
    rp = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    return sp.csr_matrix((v, c.astype(np.int32), rp), shape=(n, n))


def narrow(n: int, seed: int = 0) -> sp.csr_matrix:
    """A tridiagonal matrix plus the couplings (i, i + 3) for every fourth i counted from the END (i = n - 4, n - 8, ...), values
    ~ -U(0.2, 1): 5 n / 4 entries above the diagonal, and the last row of L has the two dependencies n - 4 and n - 2."""
    rng = np.random.default_rng(seed)
    a = np.arange(n - 1)
    b = np.arange(n - 4, -1, -4)[::-1]
    rows, cols = np.concatenate([a, b]), np.concatenate([a + 1, b + 3])
    return _spd(n, rows, cols, -rng.uniform(0.2, 1.0, rows.size))


def penta(n: int, seed: int = 0, second=None) -> sp.csr_matrix:
    """Couplings (i, i + 1) and (i, i + 2), values ~ -U(0.2, 1) (`second`: the value of every (i, i + 2) instead)."""
    rng = np.random.default_rng(seed)
    a, b = np.arange(n - 1), np.arange(n - 2)
    v1, v2 = -rng.uniform(0.2, 1.0, a.size), -rng.uniform(0.2, 1.0, b.size)
    if second is not None:
        v2 = np.full(b.size, float(second))
    return _spd(n, np.concatenate([a, b]), np.concatenate([a + 1, b + 2]), np.concatenate([v1, v2]))


def wide_row(m: int) -> sp.csr_matrix:
    """Row 0 coupled to the rows 1 .. m (column 0 of A has m entries below the diagonal), the rest a chain."""
    n = m + 4
    a = np.arange(1, n - 1)
    rows = np.concatenate([np.zeros(m, dtype=np.int64), a])
    cols = np.concatenate([np.arange(1, m + 1), a + 1])
    vals = np.concatenate([-(1.0 + 0.01 * np.arange(m)), -np.ones(a.size)])
    return _spd(n, rows, cols, vals)


def arrow(m: int) -> sp.csr_matrix:
    """The columns 0 .. m - 1 each hold one entry below the diagonal, in row m; two more rows chained behind it.  Row m of L keeps
    m entries; no column depends on its predecessor before row m."""
    n = m + 3
    rows = np.concatenate([np.arange(m), [m, m + 1]])
    cols = np.concatenate([np.full(m, m), [m + 1, m + 2]])
    return _spd(n, rows, cols, -(1.0 + 0.01 * np.arange(rows.size)))


def arrow_then_wide_column() -> sp.csr_matrix:
    """Row H = 145 of L is filled to 64 entries by the columns 0 .. 63; column 64 holds 81 candidates -- its own rows 105 .. 144
    and H, and the fill of column 0 at the rows 65 .. 104 and H -- and would keep H again: the 65th entry of row H, found where
    the columns of more than 64 candidates append."""
    n, c, h = 147, 64, 145
    r1, r2 = np.arange(65, 105), np.arange(105, 145)
    rows = [np.arange(1, 64), [0], np.zeros(r1.size, dtype=np.int64), [0], [c], np.full(r2.size, c), [h]]
    cols = [np.full(63, h), [c], r1, [h], [h], r2, [h + 1]]
    vals = [-np.ones(63), [-1.0], -0.1 * np.ones(r1.size), [-1.0], [-3.0], -np.ones(r2.size), [-1.0]]
    return _spd(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def converging(d: int, s: int, own: int = 0) -> sp.csr_matrix:
    """The columns 0 .. d - 1 each hold column c = d and s rows of their own (disjoint sets behind c); column c holds `own` further
    rows.  Every early column keeps all its entries (threshold 0), so column c meets exactly d s + own candidates."""
    c = d
    n = c + 1 + d * s + own
    rows, cols, vals = [], [], []
    for j in range(d):
        mine = c + 1 + j * s + np.arange(s)
        rows += [[j], np.full(s, j)]
        cols += [[c], mine]
        vals += [[-1.0], -(0.5 + 0.001 * (np.arange(s) + j))]
    if own:
        rows.append(np.full(own, c))
        cols.append(n - own + np.arange(own))
        vals.append(-np.ones(own))
    return _spd(n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


HUB, HUB_BELOW, HUB_ABOVE = 100, np.arange(10, 80), np.arange(110, 160)


def hub_row() -> sp.csr_matrix:
    """A chain of 200 rows and a hub row 100 coupled to 70 rows before it (20 of them by 1e-3: the threshold drops those, so row 100
    of L stays under its cap) and to 50 behind it: 122 stored entries, the diagonal the 71st, 51 of them right of the diagonal."""
    n = 200
    a = np.arange(n - 1)
    rows = np.concatenate([a, HUB_BELOW, np.full(HUB_ABOVE.size, HUB)])
    cols = np.concatenate([a + 1, np.full(HUB_BELOW.size, HUB), HUB_ABOVE])
    vals = np.concatenate([-np.ones(a.size), np.where(HUB_BELOW < 30, -1e-3, -0.5 - 0.001 * HUB_BELOW), -0.3 - 0.001 * HUB_ABOVE])
    return _spd(n, rows, cols, vals)


def tie_cut() -> sp.csr_matrix:
    """Column 1 meets seven candidates: fill of magnitude exactly 1 at the rows 2, 3, 4 (signs -, +, -; from column 0, whose
    pivot is 8: 8 * (+-8) / 64) and its own entries +1, -1, 3, 0.5 at the rows 5 .. 8.  Its count bound is 4: the 3 and three of
    the five candidates of magnitude 1 -- the rows 2, 3, 4, which came last."""
    rows = [0, 0, 0, 0, 1, 1, 1, 1]
    cols = [1, 2, 3, 4, 5, 6, 7, 8]
    vals = [8.0, 8.0, -8.0, 8.0, 1.0, -1.0, 3.0, 0.5]
    diag = [64.0, 16.0, 12.0, 12.0, 12.0, 4.0, 4.0, 8.0, 4.0]
    return _spd(9, rows, cols, vals, diag)


def cancelling() -> sp.csr_matrix:
    """Column 1's candidate at row 2 is its own entry 1 minus the fill 8 * 8 / 64: exactly 0.0; A also stores zeros at (1, 4) and
    (3, 5)."""
    rows = [0, 0, 1, 1, 1, 3, 4]
    cols = [1, 2, 2, 3, 4, 5, 5]
    vals = [8.0, 8.0, 1.0, -1.0, 0.0, 0.0, -1.0]
    diag = [64.0, 16.0, 16.0, 4.0, 4.0, 4.0]
    return _spd(6, rows, cols, vals, diag)


def two_chains(n: int = 40) -> sp.csr_matrix:
    """Couplings (i, i + 2) only: the even and the odd rows are two chains, column k never depends on column k - 1."""
    a = np.arange(n - 2)
    return _spd(n, a, a + 2, -(1.0 + 0.01 * a))


def diagonal(n: int = 130) -> sp.csr_matrix:
    return E.csr(sp.diags(np.arange(1.0, n + 1.0)))


def harness_base() -> sp.csr_matrix:
    return E.nine_point_mixed(10)


def scaled(A, factor: float) -> sp.csr_matrix:
    B = A.copy()
    B.data = B.data * factor
    return B


def _entry(A, r, c) -> int:
    k = A.indptr[r] + int(np.searchsorted(A.indices[A.indptr[r]:A.indptr[r + 1]], c))
    assert A.indices[k] == c
    return k


def with_entries(A, entries) -> sp.csr_matrix:
    B = A.copy()
    for (r, c), v in entries.items():
        B.data[_entry(B, r, c)] = v
    return B


def without_entries(A, entries):
    """(rowptr, col, val) of A without the given stored (row, col) positions."""
    A = E.csr(A)
    keep = np.ones(A.nnz, dtype=bool)
    for r, c in entries:
        keep[_entry(A, r, c)] = False
    row_of = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    rp = np.zeros(A.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(row_of[keep], minlength=A.shape[0]), out=rp[1:])
    return rp, A.indices[keep].astype(np.int32), A.data[keep].copy()


def fill_case() -> sp.csr_matrix:
    """The matrix of the storage cases: a 9-point stencil whose factor holds fill at add_fill_in = 2, threshold = 0.01."""
    return E.nine_point_mixed(12)


def reversed_rows(A):
    """(rowptr, col, val) with the entries of every row in descending column order."""
    A = E.csr(A)
    rp = A.indptr.astype(np.int32)
    ci, v = A.indices.astype(np.int32).copy(), A.data.copy()
    for i in range(A.shape[0]):
        s, e = rp[i], rp[i + 1]
        ci[s:e], v[s:e] = ci[s:e][::-1].copy(), v[s:e][::-1].copy()
    return rp, ci, v


def one_row_exchanged(A, row: int = 77):
    """(rowptr, col, val) with the diagonal entry of `row` and the entry behind it exchanged."""
    A = E.csr(A)
    rp, ci, v = A.indptr.astype(np.int32), A.indices.astype(np.int32).copy(), A.data.copy()
    k = _entry(A, row, row)
    assert k + 1 < rp[row + 1]
    ci[k], ci[k + 1] = ci[k + 1], ci[k]
    v[k], v[k + 1] = v[k + 1], v[k]
    return rp, ci, v


def lower_stripped(A, every: Optional[int]):
    """(rowptr, col, val) without every `every`-th stored entry left of the diagonal (None: without all of them)."""
    A = E.csr(A)
    C = A.tocoo()
    low = np.nonzero(C.row > C.col)[0]
    drop = low if every is None else low[::every]
    return without_entries(A, list(zip(C.row[drop], C.col[drop])))


def upper_without_mirror(A, r: int = 30, c: int = 100, v: float = -0.25):
    """(rowptr, col, val) of A plus the entry (r, c) right of the diagonal, whose mirror (c, r) is not stored."""
    A = E.csr(A)
    assert r < c and A[r, c] == 0
    B = sp.csr_matrix(A + sp.csr_matrix(([v], ([r], [c])), shape=A.shape))
    B.sort_indices()
    return B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.copy()


NEXT_AFTER_ONE = float(np.nextafter(1.0, 2.0))
W4, W8, W16 = {"DPCG_ICHOLT_WAVES": "4"}, {"DPCG_ICHOLT_WAVES": "8"}, {"DPCG_ICHOLT_WAVES": "16"}
WORKSPACE, ONE_WAVE, ONE_WAVE_LDS = {"DPCG_ICHOLT_LDS": "2"}, {"DPCG_ICHOLT_LDS": "0"}, {"DPCG_ICHOLT_LDS": "0", "DPCG_ICHOLT_REGS": "0"}
LDS_EDGE_N = 2595                  # penta(n), add_fill_in = 1: pool_cap = 3 n - 2; the LDS form's bytes fit up to this n
POOL_EDGE_N = 8160                 # penta(n), add_fill_in = 6: pool_cap = 8 n - 2 < 0xff00 up to this n


def _forms():
    out = [Case(f"narrow{n}", lambda n=n: narrow(n), 0, 0.0, form=f, facts={"last_row_dependencies": 2})
           for n, f in ((4095, 1), (4096, 1), (4097, 2))]
    out += [Case(f"penta{n}", lambda n=n: penta(n), 1, 0.1, form=f, facts={"depends_on_predecessor": min(n - 1, 8191)})
            for n, f in ((8191, 2), (8192, 2), (8193, 3))]
    out += [Case(f"penta{LDS_EDGE_N}_lds_fits", lambda: penta(LDS_EDGE_N), 1, 0.1, form=1),
            Case(f"penta{LDS_EDGE_N + 1}_lds_over", lambda: penta(LDS_EDGE_N + 1), 1, 0.1, form=2),
            Case(f"penta{POOL_EDGE_N}_pool_fits", lambda: penta(POOL_EDGE_N), 6, 0.05, form=2),
            Case(f"penta{POOL_EDGE_N + 1}_pool_over", lambda: penta(POOL_EDGE_N + 1), 6, 0.05, form=3)]
    for env in (W4, W8, W16):
        w = env["DPCG_ICHOLT_WAVES"]
        out += [Case(f"tiny{n}_w{w}", lambda n=n: E.tiny(n), 1, 0.1, env=env, form=1) for n in (1, 2, 3, 5, 17)]
        out.append(Case(f"nine_point24_w{w}", lambda: E.nine_point_mixed(24), 2, 0.01, env=env, form=1))
    return out


def _caps():
    out = [Case("wide_row64_fill0", lambda: wide_row(64), 0, 0.0, facts={"kept": (0, 64)}),
           Case("wide_row65_fill0", lambda: wide_row(65), 0, 0.0, refusal="colcap", column=0),
           Case("wide_row63_fill1", lambda: wide_row(63), 1, 0.0, facts={"kept": (0, 63), "p": (0, 64)}),
           Case("wide_row64_fill1", lambda: wide_row(64), 1, 0.0, refusal="colcap", column=0),
           Case("arrow64", lambda: arrow(64), 0, 0.0, facts={"row_entries": (64, 64)}),
           Case("arrow65", lambda: arrow(65), 0, 0.0, refusal="rowcap", column=64, facts={"row_would_keep": (65, 65)}),
           Case("arrow_then_wide_column", arrow_then_wide_column, 0, 0.0, refusal="rowcap", column=64,
                facts={"candidates_at_refusal": 81}),
           Case("converging64", lambda: converging(2, 32), 1, 0.0, facts={"candidates": (2, 64)}),
           Case("converging65", lambda: converging(2, 32, 1), 1, 0.0, retry=2, facts={"candidates": (2, 65)}),
           Case("converging256", lambda: converging(8, 32), 1, 0.0, retry=8, facts={"candidates": (8, 256)}),
           Case("converging257", lambda: converging(8, 32, 1), 1, 0.0, refusal="cand", column=8, facts={"candidates_at_refusal": 257})]
    out += [Case("converging64" + tag, lambda: converging(2, 32), 1, 0.0, env=env, facts={"candidates": (2, 64)})
            for tag, env in (("_one_wave", ONE_WAVE), ("_one_wave_lds", ONE_WAVE_LDS))]
    out += [Case("hub_row" + tag, hub_row, 1, 0.1, env=env, facts={"hub": True})
            for tag, env in (("", {}), ("_one_wave", ONE_WAVE), ("_one_wave_lds", ONE_WAVE_LDS))]
    return out


def _selection():
    return [Case("tie_cut", tie_cut, 0, 0.05, facts={"tie_cut": 1}),
            Case("tie_cut_one_wave", tie_cut, 0, 0.05, env=ONE_WAVE, facts={"tie_cut": 1}),
            Case("tie_cut_one_wave_lds", tie_cut, 0, 0.05, env=ONE_WAVE_LDS, facts={"tie_cut": 1}),
            Case("on_threshold_kept", lambda: E.tiny(17), 1, 1.0, facts={"on_bound": True, "strict_lower": 16}),
            Case("on_threshold_kept_one_wave", lambda: E.tiny(17), 1, 1.0, env=ONE_WAVE, facts={"on_bound": True, "strict_lower": 16}),
            Case("above_threshold_dropped", lambda: E.tiny(17), 1, NEXT_AFTER_ONE, facts={"strict_lower": 0}),
            Case("threshold_1e300", lambda: E.nine_point_mixed(8), 1, 1e300, facts={"strict_lower": 0}),
            Case("threshold_inf", lambda: E.nine_point_mixed(8), 1, float("inf"), facts={"strict_lower": 0}),
            Case("threshold_inf_one_wave", lambda: E.nine_point_mixed(8), 1, float("inf"), env=ONE_WAVE, facts={"strict_lower": 0}),
            Case("cancelling_thr0", cancelling, 0, 0.0, facts={"zero_candidate": (1, 2), "stored_zeros_in_L": True}),
            Case("cancelling_thr0_one_wave", cancelling, 0, 0.0, env=ONE_WAVE, facts={"zero_candidate": (1, 2), "stored_zeros_in_L": True}),
            Case("cancelling_thr01", cancelling, 0, 0.1, facts={"zero_candidate": (1, 2)}),
            Case("diagonal130", diagonal, 1, 0.1, facts={"strict_lower": 0}),
            Case("two_chains", two_chains, 1, 0.1, facts={"never_depends_on_predecessor": True})]


def _nan_base() -> sp.csr_matrix:
    return penta(40, seed=3)


def _values():
    up, down = 4.0 ** 100, 4.0 ** -100
    return [Case("harness", harness_base, 1, 0.1),
            Case("harness_times_4e100", lambda: scaled(harness_base(), up), 1, 0.1, facts={"scaled_from": ("harness", 2.0 ** 100)}),
            Case("harness_times_4e-100", lambda: scaled(harness_base(), down), 1, 0.1, facts={"scaled_from": ("harness", 2.0 ** -100)}),
            Case("harness_times_4e100_one_wave", lambda: scaled(harness_base(), up), 1, 0.1, env=ONE_WAVE,
                 facts={"scaled_from": ("harness", 2.0 ** 100)}),
            Case("harness_1e160", lambda: scaled(harness_base(), 1e160), 1, 0.1, facts={"squares_overflow": True}),
            Case("harness_1e160_one_wave", lambda: scaled(harness_base(), 1e160), 1, 0.1, env=ONE_WAVE, facts={"squares_overflow": True}),
            Case("harness_1e-160", lambda: scaled(harness_base(), 1e-160), 1, 0.1, facts={"squares_underflow": True}),
            Case("harness_1e-160_one_wave", lambda: scaled(harness_base(), 1e-160), 1, 0.1, env=ONE_WAVE, facts={"squares_underflow": True}),
            Case("nan_below_diagonal", lambda: with_entries(_nan_base(), {(20, 21): np.nan, (21, 20): np.nan}), 1, 0.1,
                 refusal="pivot", column=21),
            Case("inf_below_diagonal", lambda: with_entries(_nan_base(), {(20, 21): np.inf, (21, 20): np.inf}), 1, 0.1,
                 refusal="pivot", column=21),
            Case("nan_on_diagonal", lambda: with_entries(_nan_base(), {(20, 20): np.nan}), 1, 0.1, refusal="pivot", column=20),
            Case("nan_on_diagonal_one_wave_lds", lambda: with_entries(_nan_base(), {(20, 20): np.nan}), 1, 0.1, env=ONE_WAVE_LDS,
                 refusal="pivot", column=20),
            # an inf pivot is a pivot: L_kk = inf, zeros (signed) below it -- the restatement refuses nothing, nor does the device
            Case("inf_on_diagonal", lambda: with_entries(_nan_base(), {(20, 20): np.inf}), 1, 0.1, nonfinite=True),
            Case("missing_diagonal", lambda: without_entries(_nan_base(), [(20, 20)]), 1, 0.1, refusal="nodiag", column=20),
            Case("missing_diagonal_one_wave", lambda: without_entries(_nan_base(), [(20, 20)]), 1, 0.1, env=ONE_WAVE,
                 refusal="nodiag", column=20)]


def _storage():
    out = []
    for tag, env in (("", {}), ("_workspace", WORKSPACE), ("_one_wave", ONE_WAVE), ("_one_wave_lds", ONE_WAVE_LDS)):
        out += [Case("reversed_rows" + tag, lambda: reversed_rows(fill_case()), 2, 0.01, env=env, facts={"same_as": "sorted"}),
                Case("one_row_exchanged" + tag, lambda: one_row_exchanged(fill_case()), 2, 0.01, env=env, facts={"same_as": "sorted"})]
    out += [Case("sorted", fill_case, 2, 0.01, facts={"has_fill": True}),
            Case("sorted_workspace", fill_case, 2, 0.01, env=WORKSPACE),
            # two entries fewer: the pool bound still holds what is staged.  Every third: it does not, the one-wave kernel factors.
            Case("lower_two_stripped", lambda: without_entries(fill_case(), [(50, 49), (90, 78)]), 2, 0.01, facts={"same_as": "sorted"}),
            Case("lower_third_stripped", lambda: lower_stripped(fill_case(), 3), 2, 0.01, retry=0, facts={"same_as": "sorted"}),
            Case("upper_only", lambda: lower_stripped(fill_case(), None), 2, 0.01, retry=0, facts={"same_as": "sorted"}),
            Case("upper_only_one_wave", lambda: lower_stripped(fill_case(), None), 2, 0.01, env=ONE_WAVE, facts={"same_as": "sorted"}),
            Case("upper_without_mirror", lambda: upper_without_mirror(fill_case()), 2, 0.01),
            Case("upper_without_mirror_workspace", lambda: upper_without_mirror(fill_case()), 2, 0.01, env=WORKSPACE)]
    return out


FORM_CASES = tuple(_forms())
CASES = FORM_CASES + tuple(_caps()) + tuple(_selection()) + tuple(_values()) + tuple(_storage())
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
FORM_PAIRS = (("narrow4096", "narrow4097"), ("penta8192", "penta8193"), (f"penta{LDS_EDGE_N}_lds_fits", f"penta{LDS_EDGE_N + 1}_lds_over"),
              (f"penta{POOL_EDGE_N}_pool_fits", f"penta{POOL_EDGE_N + 1}_pool_over"))

# the restatement's single-defect variants (oracle.ICHOLT_DEFECTS) and a case whose factor each one changes
MUTANT_CAUGHT_BY = {
    "ties_to_larger_row": "tie_cut",
    "drop_on_equal": "on_threshold_kept",
    "norm_with_diagonal": "on_threshold_kept",
    "dependencies_descending": "sorted",
    "count_without_fill": "harness",
    "scale_by_unreduced_diagonal": "harness",
}

# ---- life cycle (tests/test_icholt_edges_gpu.py runs these sequences; the host test checks what they rest on) -----------------
THRESHOLD_CROSSING = dict(n=60, add_fill_in=1, threshold=0.5, before=-0.1, after=-0.9)     # penta(n, second=...): (i, i + 2) dropped, then kept
REPEAT_CASES = ("nine_point24_w4", "nine_point24_w8", "nine_point24_w16", "sorted_workspace")
