"""The table of tests/icholt_edge_cases.py means what it says (CPU only): every accepted case factors and every refused case raises
the named kind at the named column in the restatement (oracle.icholt); the counts a case is built for -- 64 | 65 | 256 | 257
candidates, 64 kept entries and a 65th refused, a hub row of more than 64 entries, a count bound that cuts through a tie, a candidate
exactly on the threshold, squares that overflow or vanish while the factor stays finite -- are what the restatement's `stats` report;
the dispatcher's limits predict the form each boundary case is in the table for; and every single-defect variant of the restatement
changes the factor of the case the table names for it, so a device routine with that defect could not pass the GPU file."""

import numpy as np
import pytest
import scipy.sparse as sp

import icholt_edge_cases as X
from oracle import oracle as O

_CACHE = {}


def restated(name):
    """(A, L or the IcholtError, stats) of a table case: computed once, never written to."""
    if name not in _CACHE:
        c = X.CASE_BY_NAME[name]
        A = X.as_csr(c.matrix())
        stats = {}
        try:
            with np.errstate(all="ignore"):
                L = O.icholt(A, c.add_fill_in, c.threshold, stats=stats)
            L.data.setflags(write=False)
        except O.IcholtError as e:
            L = e
        _CACHE[name] = (A, L, stats)
    return _CACHE[name]


def _bits(L):
    return L.indptr.tobytes() + L.indices.tobytes() + L.data.tobytes()


def _has_fill(L, A):
    """L stores an entry below the diagonal where A stores none."""
    P = (sp.tril(L, -1) != 0).astype(np.int64)
    return (P - P.multiply(A != 0)).nnz > 0


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_case_is_what_the_table_says(case):
    A, L, stats = restated(case.name)
    n = A.shape[0]
    rp, ci, _ = X.arrays(case.matrix())
    form, waves, retry, cap = X.predict(rp, ci, case.add_fill_in, case.env)
    if case.refusal is not None:
        assert isinstance(L, O.IcholtError) and (L.kind, L.column) == (case.refusal, case.column)
    else:
        assert not isinstance(L, Exception), L
        assert sp.triu(L, 1).nnz == 0 and (L.diagonal() > 0).all()
        assert np.isfinite(L.data).all() != case.nonfinite
        if case.form is not None:
            assert form == case.form
        if case.retry == 0:
            assert retry == 0                                       # (the staging's retry is the one the limits predict)
        elif case.retry is None:
            assert retry is None
        else:
            assert form != 3 and max(stats["candidates"]) > X.CAP and stats["candidates"].index(max(stats["candidates"])) == case.retry
            assert [k for k in range(n) if stats["candidates"][k] > X.CAP] == [case.retry]
    f = case.facts
    if "candidates" in f:
        k, count = f["candidates"]
        assert stats["candidates"][k] == count and max(stats["candidates"]) == count
    if "candidates_at_refusal" in f:                                # (stats stop at the refused column: count them from A and L's rule)
        with pytest.raises(O.IcholtError):
            O.icholt(A, case.add_fill_in, case.threshold, cand_cap=f["candidates_at_refusal"] - 1, row_cap=10 ** 6)
        more = {}
        O.icholt(A, case.add_fill_in, case.threshold, cand_cap=f["candidates_at_refusal"], row_cap=10 ** 6, stats=more)
        assert more["candidates"][case.column] == f["candidates_at_refusal"]
    if "kept" in f:
        k, count = f["kept"]
        assert stats["kept"][k] == count == np.count_nonzero(sp.tril(L, -1).tocsc()[:, k].toarray())
    if "p" in f:
        assert stats["p"][f["p"][0]] == f["p"][1]
    if "row_entries" in f:
        row, count = f["row_entries"]
        assert L.indptr[row + 1] - L.indptr[row] - 1 == count == X.CAP and np.diff(L.indptr).max() - 1 == count
    if "row_would_keep" in f:
        row, count = f["row_would_keep"]
        free = O.icholt(A, case.add_fill_in, case.threshold, row_cap=10 ** 6)
        assert free.indptr[row + 1] - free.indptr[row] - 1 == count == X.CAP + 1
    if f.get("hub"):
        h = X.HUB
        row = A.indices[A.indptr[h]:A.indptr[h + 1]]
        assert row.size > X.CAP and np.count_nonzero(row > h) <= X.CAP and int(np.searchsorted(row, h)) >= X.CAP
        assert L.indptr[h + 1] - L.indptr[h] - 1 <= X.CAP and max(stats["candidates"]) <= X.CAP
        assert L.indptr[h + 1] - L.indptr[h] - 1 >= 50             # (the hub's large couplings are kept: a row of L with many dependencies)
    if "tie_cut" in f:
        k = f["tie_cut"]
        assert stats["tie_cut"][k] and stats["passed"][k] > stats["p"][k]
        rows = L.tocsc()[:, k].nonzero()[0]
        assert list(rows) == [1, 2, 3, 4, 7]                       # the 3 and the three SMALLER rows of the five tied ones
        assert len({np.sign(L[r, k]) for r in (2, 3, 4)}) == 2      # mixed signs inside the tie
    if f.get("on_bound"):
        assert all(stats["on_bound"][:-1]) and stats["kept"][:-1] == [1] * (n - 1)
    if "strict_lower" in f:
        assert sp.tril(L, -1).nnz == f["strict_lower"]
    if "zero_candidate" in f:
        k, r = f["zero_candidate"]
        assert stats["candidates"][k] == 3 and np.count_nonzero(A.data == 0.0) == 4
        if f.get("stored_zeros_in_L"):
            pos = L.indptr[r] + list(L.indices[L.indptr[r]:L.indptr[r + 1]]).index(k)
            assert L.data[pos] == 0.0 and L.nnz == 13
        else:
            assert L[r, k] == 0 and k not in L.indices[L.indptr[r]:L.indptr[r + 1]]
    if f.get("never_depends_on_predecessor"):
        C = sp.tril(L, -1).tocoo()
        assert C.nnz > 0 and not (C.row - C.col == 1).any()
    if "last_row_dependencies" in f:
        assert L.indptr[n] - L.indptr[n - 1] - 1 >= f["last_row_dependencies"]
        assert (np.diff(L.indptr)[-8:] >= 3).sum() >= 2            # columns near the end with two dependencies
    if "depends_on_predecessor" in f:
        k = f["depends_on_predecessor"]
        assert L[k, k - 1] != 0
    if "scaled_from" in f:
        base, factor = f["scaled_from"]
        Lb = restated(base)[1]
        assert np.array_equal(L.indptr, Lb.indptr) and np.array_equal(L.indices, Lb.indices)
        assert np.array_equal((Lb.data * factor).view(np.uint64), L.data.view(np.uint64)) and np.isfinite(L.data).all()
        assert all(stats["squares_finite"])                         # nothing overflowed or went subnormal on the way
    if f.get("squares_overflow"):
        assert not any(stats["squares_finite"][:-1]) and np.isfinite(L.data).all() and sp.tril(L, -1).nnz == 0
    if f.get("squares_underflow"):
        assert not any(stats["squares_finite"][:-1]) and np.isfinite(L.data).all() and sp.tril(L, -1).nnz > 0
    if f.get("same_as"):
        assert _bits(L) == _bits(restated(f["same_as"])[1])
        assert case.name.startswith(("lower", "upper")) or not X.as_csr(case.matrix()).has_sorted_indices
    if f.get("has_fill"):
        assert _has_fill(L, A)


def test_form_boundary_pairs_differ_by_the_limit_they_are_named_for():
    for a, b in X.FORM_PAIRS:
        ca, cb = X.CASE_BY_NAME[a], X.CASE_BY_NAME[b]
        pa = X.predict(*X.arrays(ca.matrix())[:2], ca.add_fill_in, ca.env)
        pb = X.predict(*X.arrays(cb.matrix())[:2], cb.add_fill_in, cb.env)
        assert pa[0] != pb[0] and (pa[0], pb[0]) == (ca.form, cb.form) and pa[2] is None and pb[2] is None
    n = X.LDS_EDGE_N
    assert X.lds_bytes(n, X.pool_cap(n, 5 * n - 6, 1), 4) + 64 <= X.LDS_BYTES < X.lds_bytes(n + 1, X.pool_cap(n + 1, 5 * n - 1, 1), 4) + 64
    n = X.POOL_EDGE_N
    assert X.pool_cap(n, 5 * n - 6, 6) < X.POOL_LIMIT <= X.pool_cap(n + 1, 5 * n - 1, 6) and n + 1 <= X.WORKSPACE_MAX_ROWS
    # the limits here are the ones the header documents and the dispatcher applies
    import pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    header = (root / "include" / "dpcg.h").read_text()
    source = (root / "deeppreconditioning_amd" / "csrc" / "dpcg_icholt.hip").read_text()
    for text in ("n <= 4096", "n <= 8192", "pool_cap < 0xff00", "160 KiB", "4096 + 256 (W + 8) + 14 P + 2 (P mod 2) + 18 R",
                 "(nnz - n + 1) / 2 + n add_fill_in + 1", "int dpcg_get_icholt_info(dpcg_handle_t h, int32_t out[4]);"):
        assert text in header, text
    for text in ("kLdsMaxRows = 4096", "kGmMaxRows = 8192", "pool_cap < 0xff00", "160 * 1024",
                 "(A.nnz - n + 1) / 2 + n * (int64_t)add_fill_in + 1"):
        assert text in source, text


@pytest.mark.parametrize("defect", O.ICHOLT_DEFECTS)
def test_every_defect_of_the_rule_changes_a_named_case(defect):
    """`scale_by_unreduced_diagonal` is the restatement's reading of "the diagonal reduced after the candidates": the candidates are
    divided by the square root of the diagonal as A stores it, the reduction reaches L_kk only."""
    name = X.MUTANT_CAUGHT_BY[defect]
    c = X.CASE_BY_NAME[name]
    A, L, _ = restated(name)
    try:
        with np.errstate(all="ignore"):
            Lm = O.icholt(A, c.add_fill_in, c.threshold, defect=defect)
    except O.IcholtError:
        return                                                      # (a refusal where the rule factors is a difference too)
    assert _bits(Lm) != _bits(L), f"{defect} is not seen by {name}"


def test_life_cycle_sequences_rest_on_what_they_claim():
    t = X.THRESHOLD_CROSSING
    before = O.icholt(X.penta(t["n"], second=t["before"]), t["add_fill_in"], t["threshold"])
    after = O.icholt(X.penta(t["n"], second=t["after"]), t["add_fill_in"], t["threshold"])
    A1, A2 = X.penta(t["n"], second=t["before"]), X.penta(t["n"], second=t["after"])
    assert np.array_equal(A1.indptr, A2.indptr) and np.array_equal(A1.indices, A2.indices)      # update_values: the same pattern
    assert before.nnz == 2 * t["n"] - 1 and sp.tril(before, -2).nnz == 0 and sp.tril(after, -2).nnz > 20   # (i + 2, i) entries appear
    for name in X.REPEAT_CASES:
        c = X.CASE_BY_NAME[name]
        rp, ci, _ = X.arrays(c.matrix())
        assert X.predict(rp, ci, c.add_fill_in, c.env)[0] in (1, 2) and restated(name)[2]["candidates"]
        L = restated(name)[1]
        assert _has_fill(L, X.as_csr(c.matrix()))                                                # a pipeline case WITH fill
