"""Named, seeded inputs of tests/test_coo_edges_host.py and tests/test_coo_edges_gpu.py: the training-path COO kernels and COO -> CSR at
the sizes where they take another path.  Test infrastructure, not product.

Launch geometry, as written in launch_batched_coo_spmv / _edge / _spmm / _sddmm at the end of deeppreconditioning_amd/csrc/dpcg_setup.hip
(kBlock lanes a block; the grid is capped, the kernels stride over the rest):
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import coo_restatement as R

BLOCK = 256                      # kBlock
WAVE = 64
SPMV_CAP_BLOCKS = 4096           # one lane per triple
EDGE_CAP_BLOCKS = 4096           # one lane per triple
SPMM_CAP_BLOCKS = 16384          # one lane per (triple, column)
SDDMM_CAP_BLOCKS = 8192          # one wave per triple: 32 768 waves
SPMV_CAP = SPMV_CAP_BLOCKS * BLOCK
EDGE_CAP = EDGE_CAP_BLOCKS * BLOCK
SPMM_CAP = SPMM_CAP_BLOCKS * BLOCK
SDDMM_CAP = SDDMM_CAP_BLOCKS * BLOCK // WAVE

TRANSPOSES = (False, True)
OPS = ("spmv", "edge", "spmm", "sddmm")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    idx: np.ndarray              # (nnz, 3) int32 (batch, row, col)
    feat: np.ndarray             # (nnz,) float32
    batch: int
    dof: int
    widths: tuple                # the panel widths spmm and sddmm run with
    poisoned: tuple = ()         # rows of vec / panel that hold inf and NaN (explicit_zeros)

    @property
    def nnz(self):
        return len(self.feat)


def values(rng, shape) -> np.ndarray:
    """fp32-exact, in +-[0.5, 2]: a product of two is exact in fp64 and lies in [0.25, 4] -- no term is small"""
    return (rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _random_case(name, seed, nnz, batch, dof, widths) -> Case:
    rng = np.random.default_rng(seed)
    idx = np.column_stack((rng.integers(0, batch, nnz), rng.integers(0, dof, nnz), rng.integers(0, dof, nnz))).astype(np.int32)
    return Case(name, idx, values(rng, nnz), batch, dof, tuple(widths))


def _batch_offsets() -> Case:
    """batch = 5: samples 0 and 3 are empty, sample 2 holds one triple at (dof - 1, 0), samples 1 and 4 a random pattern each"""
    rng = np.random.default_rng(105)
    dof, parts = 11, []
    for b, count in ((1, 40), (4, 33)):
        parts.append(np.column_stack((np.full(count, b), rng.integers(0, dof, count), rng.integers(0, dof, count))))
    parts.insert(1, np.array([[2, dof - 1, 0]]))
    idx = np.vstack(parts).astype(np.int32)
    return Case("batch_offsets", idx, values(rng, len(idx)), 5, dof, (1, 5))


def _all_duplicates() -> Case:
    rng = np.random.default_rng(106)
    idx = np.tile(np.array([[1, 3, 5]], dtype=np.int32), (300, 1))
    return Case("all_duplicates", idx, values(rng, 300), 2, 8, (3,))


INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def _out_of_range() -> Case:
    """a valid pattern with triples out of range in between: b = -1, b = batch, r = dof, c = -1, c = dof as asked, and r = -1 and the
    two ends of int32 besides"""
    valid = _random_case("valid", 107, 60, 2, 9, (1, 4))
    batch, dof = valid.batch, valid.dof
    bad = [(-1, 1, 2), (batch, 1, 2), (0, dof, 2), (1, 3, -1), (1, 3, dof), (0, -1, 4), (0, INT32_MAX, 1), (1, 2, INT32_MIN)]
    rng = np.random.default_rng(108)
    idx, feat = list(map(tuple, valid.idx)), list(valid.feat)
    for k, triple in enumerate(bad):
        at = 0 if k == 0 else len(idx) if k == 1 else int(rng.integers(1, len(idx)))     # the first, the last, and in between
        idx.insert(at, triple)
        feat.insert(at, values(rng, ())[()])
    return Case("out_of_range", np.array(idx, dtype=np.int32), np.array(feat, dtype=np.float32), batch, dof, valid.widths)


def valid_part(case: Case) -> tuple:
    """(mask of the triples in range, the case without the others)"""
    _, _, _, ok = R._triples(case.idx, case.batch, case.dof, False)
    return ok, dataclasses.replace(case, name=case.name + ":valid", idx=case.idx[ok], feat=case.feat[ok])


def _explicit_zeros() -> Case:
    """rows Z = {2, 7} of vec and of the panel hold inf and NaN.  Triples with a non-zero feature stay clear of Z in row and column;
    triples with feature +0 or -0 touch Z in the column (read with transpose = 0), in the row (read with transpose = 1) or in both."""
    rng = np.random.default_rng(109)
    batch, dof, Z = 2, 12, (2, 7)
    clear = np.array([i for i in range(dof) if i not in Z])
    count = 70
    idx = np.column_stack((rng.integers(0, batch, count), rng.choice(clear, count), rng.choice(clear, count)))
    feat = values(rng, count)
    zeros = [(0, 1, 2), (0, 2, 1), (0, 7, 7), (1, 5, 7), (1, 7, 5), (1, 2, 7), (0, 1, 7), (1, 2, 3)]
    zfeat = np.array([0.0, -0.0] * (len(zeros) // 2), dtype=np.float32)
    at = rng.permutation(count + len(zeros))
    idx = np.vstack((idx, np.array(zeros)))[at].astype(np.int32)
    feat = np.concatenate((feat, zfeat))[at]
    return Case("explicit_zeros", idx, feat, batch, dof, (1, 5), poisoned=Z)


CASES = {
    "stride_spmv": lambda: _random_case("stride_spmv", 101, SPMV_CAP + 257, 2, 4096, (1,)),
    "stride_edge": lambda: _random_case("stride_edge", 111, EDGE_CAP + 257, 2, 4096, (1,)),
    "stride_sddmm": lambda: _random_case("stride_sddmm", 102, SDDMM_CAP + 5, 2, 512, (3,)),
    "stride_spmm": lambda: _random_case("stride_spmm", 103, 65537, 2, 2048, (65,)),
    "widths": lambda: _random_case("widths", 104, 400, 3, 37, (1, 2, 63, 64, 65, 128, 130)),
    "batch_offsets": _batch_offsets,
    "all_duplicates": _all_duplicates,
    "out_of_range": _out_of_range,
    "explicit_zeros": _explicit_zeros,
    "empty": lambda: Case("empty", np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.float32), 2, 5, (1, 4)),
}
# the cases whose gradients the autograd functions are checked on (the upstream gradient takes the place of vec / panel)
GRAD_CASES = ("stride_spmm", "widths", "batch_offsets", "all_duplicates")


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return CASES[name]()


def _seed(name: str, ncols: int) -> int:
    return 1000 * (list(CASES).index(name) + 1) + ncols


def _poison(c: Case, x: np.ndarray) -> np.ndarray:
    """inf, -inf and NaN into the rows c.poisoned of every sample"""
    flat = x.reshape(c.batch, c.dof, -1)
    for n, row in enumerate(c.poisoned):
        for j in range(flat.shape[2]):
            flat[:, row, j] = (np.inf, np.nan, -np.inf)[(n + j) % 3]
    return x


@functools.lru_cache(maxsize=None)
def vectors(name: str) -> tuple:
    """(vec, g), float32 (batch, dof): the vector spmv multiplies, and the upstream gradient (edge's `a`); g is always finite"""
    c = case(name)
    rng = np.random.default_rng(_seed(name, 0))
    vec, g = values(rng, (c.batch, c.dof)), values(rng, (c.batch, c.dof))
    return _poison(c, vec), g


@functools.lru_cache(maxsize=None)
def panels(name: str, ncols: int) -> tuple:
    """(panel, g), float32 (batch, dof, ncols): what spmm multiplies, and the upstream gradient (sddmm's `g`); g is always finite"""
    c = case(name)
    rng = np.random.default_rng(_seed(name, ncols))
    panel, g = values(rng, (c.batch, c.dof, ncols)), values(rng, (c.batch, c.dof, ncols))
    return _poison(c, panel), g


@functools.lru_cache(maxsize=None)
def restated(name: str, op: str, transpose: bool, ncols: int = 0, upstream: bool = False) -> R.Result:
    """The restatement of `op` on a case.  upstream: the upstream gradient takes the place of vec / panel (what the backward pass of
    the autograd functions computes with the same kernel)."""
    c = case(name)
    return _restate(c, name, op, transpose, ncols, upstream)


def _restate(c: Case, name: str, op: str, transpose: bool, ncols: int, upstream: bool, skip=None) -> R.Result:
    if op in ("spmv", "edge"):
        vec, g = vectors(name)
        if op == "spmv":
            return R.spmv(c.idx, c.feat, g if upstream else vec, c.batch, c.dof, transpose, skip=skip)
        return R.edge(c.idx, g, vec, c.batch, c.dof, transpose, skip=skip)
    panel, g = panels(name, ncols)
    if op == "spmm":
        return R.spmm(c.idx, c.feat, g if upstream else panel, c.batch, c.dof, ncols, transpose, skip=skip)
    return R.sddmm(c.idx, g, panel, c.batch, c.dof, ncols, transpose, skip=skip)


def every_restated(name: str):
    """(label, Result) for every operator, transpose and width a case runs with, and the gradients' where they are checked"""
    c = case(name)
    for op in OPS:
        for ncols in (c.widths if op in ("spmm", "sddmm") else (0,)):
            for transpose in TRANSPOSES:
                for upstream in ((False, True) if name in GRAD_CASES and op in ("spmv", "spmm") else (False,)):
                    label = f"{name} {op}{f'[{ncols}]' if ncols else ''} transpose={int(transpose)}{' upstream' if upstream else ''}"
                    yield label, restated(name, op, transpose, ncols, upstream)


# ---- mutants of the restatement -----------------------------------------------------------------------------------------------------
MUTANTS = ("batch offset b*dof replaced by 0", "row and column swapped without transpose", "last element of the stride loop dropped",
           "one duplicate dropped", "panel columns c >= 64 dropped")


# the operators the table of profiles/coo_edges.md mutates on the large cases (on every other case: all four)
MUTANT_OPS = {"stride_spmv": ("spmv",), "stride_edge": ("edge",), "stride_sddmm": ("sddmm",), "stride_spmm": ("spmm", "sddmm")}


def first_duplicate(c: Case) -> int:
    """storage position of the second triple of the first (b, r, c) that occurs twice, -1 if none does"""
    _, first, inverse = np.unique(c.idx, axis=0, return_index=True, return_inverse=True)
    again = np.nonzero(first[inverse.reshape(-1)] != np.arange(c.nnz))[0]
    return int(again[0]) if len(again) else -1


def mutated(name: str, op: str, transpose: bool, ncols: int, which: str):
    """the restatement of `op` on a case with one defect built in, or None where the case cannot show it"""
    c = case(name)
    if c.nnz == 0:
        return None
    if which == MUTANTS[0]:
        if c.batch < 2:
            return None
        _, _, _, ok = R._triples(c.idx, c.batch, c.dof, False)
        flat = c.idx.copy()
        flat[ok, 0] = 0                                  # every valid triple reads and writes sample 0
        return _restate(dataclasses.replace(c, idx=flat), name, op, transpose, ncols, False)
    if which == MUTANTS[1]:
        return _restate(c, name, op, not transpose, ncols, False)
    if which == MUTANTS[2]:
        if op == "spmm":                                 # one lane per (triple, column): the last column of the last triple
            skip = np.zeros((c.nnz, ncols), dtype=bool)
            skip[-1, -1] = True
        else:
            skip = np.zeros(c.nnz, dtype=bool)
            skip[-1] = True
        return _restate(c, name, op, transpose, ncols, False, skip=skip)
    if which == MUTANTS[3]:
        k = first_duplicate(c)
        if k < 0:
            return None
        skip = np.zeros(c.nnz, dtype=bool)
        skip[k] = True
        return _restate(c, name, op, transpose, ncols, False, skip=skip)
    if which == MUTANTS[4]:
        if op not in ("spmm", "sddmm") or ncols <= 64:
            return None
        skip = np.zeros((c.nnz, ncols), dtype=bool)
        skip[:, 64:] = True
        return _restate(c, name, op, transpose, ncols, False, skip=skip)
    raise KeyError(which)


def distance(true: R.Result, other) -> float:
    """the largest |other - true| over the outputs in units of true's bound gamma_m S (inf where the bound is 0 and they differ); an
    output that is inf or NaN in `true` has to be the same inf, or a NaN, in `other` (an array, or another Result)"""
    other = other.value if isinstance(other, R.Result) else np.asarray(other, dtype=np.float64)
    t, o, bound = true.value.reshape(-1), other.reshape(-1), true.bound().reshape(-1)
    finite = np.isfinite(t)
    if not np.array_equal(np.isnan(t), np.isnan(o)) or not np.array_equal(t[~finite & ~np.isnan(t)], o[~finite & ~np.isnan(t)]):
        return np.inf
    diff = np.abs(o[finite] - t[finite])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff > 0, diff / bound[finite], 0.0)
    return float(ratio.max(initial=0.0))


# ---- COO -> CSR ------------------------------------------------------------------------------------------------------------------------
CANCELLING = (1e16, 1.0, -1e16, 1.0)     # added front to back, a run of these differs from the same run added in any other order
RUN_LENGTHS = (1, 2, 7, 64)


def _storage_order():
    """40 keys for each run length, values from CANCELLING (starting at another place for every key), all 2960 entries shuffled:
    equal keys lie hundreds of entries apart, and their order has to survive every pass of the radix sort"""
    rng = np.random.default_rng(201)
    n = 1000
    cells = rng.choice(n * n, size=40 * len(RUN_LENGTHS), replace=False)
    rows, cols, vals = [], [], []
    for k, cell in enumerate(cells):
        length = RUN_LENGTHS[k % len(RUN_LENGTHS)]
        rows += [cell // n] * length
        cols += [cell % n] * length
        vals += [CANCELLING[(k // len(RUN_LENGTHS) + j) % 4] * (1.0 + 0.25 * (j % 3)) for j in range(length)]
    at = rng.permutation(len(rows))
    return np.array(rows)[at], np.array(cols)[at], np.array(vals)[at], n


def _with_edge_row(n, seed):
    """integer values on random cells of an n x n matrix whose last row and last column are both used"""
    rng = np.random.default_rng(seed)
    count = 400
    rows, cols = rng.integers(0, n, count), rng.integers(0, n, count)
    rows[:4], cols[:4] = (n - 1, n - 1, 0, n - 1), (n - 1, 0, n - 1, n - 1)
    return rows, cols, rng.integers(-8, 9, count).astype(np.float64), n


def _sorted(reverse):
    rng = np.random.default_rng(204)
    n, count = 90, 1500
    rows, cols = rng.integers(0, n, count), rng.integers(0, n, count)
    order = np.lexsort((cols, rows))
    if reverse:
        order = order[::-1]
    return rows[order], cols[order], rng.integers(-8, 9, count).astype(np.float64), n


def _integers():
    rng = np.random.default_rng(205)
    n, count = 500, 6000
    return rng.integers(0, n, count), rng.integers(0, n, count), rng.integers(-8, 9, count).astype(np.float64), n


COO_CASES = {
    "storage_order": _storage_order,
    "n1": lambda: (np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64), np.array([0.1, 1e16, 0.2, -1e16, 0.3, 1.0]), 1),
    "n256": lambda: _with_edge_row(256, 202),
    "n257": lambda: _with_edge_row(257, 203),
    "one_run": lambda: (np.full(5000, 3), np.full(5000, 2), np.array([CANCELLING[j % 4] * (1.0 + 0.25 * (j % 3)) for j in range(5000)]), 5),
    "sorted": lambda: _sorted(False),
    "reverse_sorted": lambda: _sorted(True),
    "nnz1": lambda: (np.array([4]), np.array([1]), np.array([0.1]), 6),
    "integers": _integers,
}
INTEGER_COO_CASES = ("n256", "n257", "sorted", "reverse_sorted", "integers")
STORAGE_ORDER_COO_CASES = ("storage_order", "n1", "one_run")


@functools.lru_cache(maxsize=None)
def coo_case(name: str):
    rows, cols, vals, n = COO_CASES[name]()
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64), int(n)


@functools.lru_cache(maxsize=None)
def coo_restated(name: str, stable: bool = True):
    return R.coo_to_csr(*coo_case(name), stable=stable)
