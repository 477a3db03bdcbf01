"""What tests/test_coo_edges_gpu.py relies on, asserted on the CPU from the numpy restatement (tests/coo_restatement.py) and the cases
(tests/coo_edge_cases.py) alone: that the restatement agrees with an independent computation, that every case reaches the code it
claims to reach, that the a-priori bound gamma_m S the GPU results are held to lies below a quarter of the smallest term of every output
(a dropped or misplaced term cannot hide in it), and that the restatement with one defect built in lies at least 10 bounds away on a
case named here.  The distances are tabulated in profiles/coo_edges.md (tools/coo_edges_probe.py)."""

import numpy as np
import pytest
import scipy.sparse as sp

import coo_edge_cases as C
import coo_restatement as R

LD = np.longdouble
DENSE_LIMIT = 512            # dof up to which the independent check builds the dense matrices


# ---- 1. the restatement against an independent computation ---------------------------------------------------------------------------
def _in_range(c):
    return np.array([0 <= b < c.batch and 0 <= r < c.dof and 0 <= s < c.dof for b, r, s in c.idx.tolist()], dtype=bool).reshape(-1)


def _dense(c, transpose):
    ok = _in_range(c)
    D = np.zeros((c.batch, c.dof, c.dof), dtype=LD)
    b, r, s = (c.idx[ok, i].astype(np.int64) for i in range(3))
    np.add.at(D, (b, r, s), c.feat[ok].astype(LD))
    return (D.transpose(0, 2, 1) if transpose else D), ok, b, (s if transpose else r), (r if transpose else s)


def _agrees(res, want, label):
    slack = 4.0 * np.maximum(res.m, 1) * 2.0 ** -53 * res.S          # an fp64 sum of m terms against a longdouble one
    err = np.abs(res.value.astype(LD) - want.reshape(res.value.shape)).astype(np.float64)
    assert np.all(err <= slack), (label, float(err.max()))


@pytest.mark.parametrize("name", [n for n in C.CASES if n != "explicit_zeros"])
def test_restatement_matches_longdouble_products(name):
    c = C.case(name)
    vec, g = C.vectors(name)
    for transpose in C.TRANSPOSES:
        if c.dof <= DENSE_LIMIT:
            D, ok, b, r, s = _dense(c, transpose)
            _agrees(C.restated(name, "spmv", transpose), np.einsum("bij,bj->bi", D, vec.astype(LD)), (name, "spmv", transpose))
            e = np.zeros(c.nnz, dtype=LD)
            e[ok] = (g.astype(LD)[:, :, None] * vec.astype(LD)[:, None, :])[b, r, s]
            assert np.array_equal(C.restated(name, "edge", transpose).value.astype(LD), e)       # one product: exact in fp64
            for ncols in c.widths:
                panel, gp = C.panels(name, ncols)
                _agrees(C.restated(name, "spmm", transpose, ncols), D @ panel.astype(LD), (name, "spmm", ncols, transpose))
                full = np.einsum("bik,bjk->bij", gp.astype(LD), panel.astype(LD))              # <g[b, i, :], panel[b, j, :]>
                d = np.zeros(c.nnz, dtype=LD)
                d[ok] = full[b, r, s]
                _agrees(C.restated(name, "sddmm", transpose, ncols), d, (name, "sddmm", ncols, transpose))
        else:                # too large for dense matrices: the same sums scattered in longdouble, straight onto the outputs
            b = c.idx[:, 0].astype(np.int64)
            r, s = (c.idx[:, 2 if transpose else 1].astype(np.int64), c.idx[:, 1 if transpose else 2].astype(np.int64))
            y = np.zeros((c.batch, c.dof), dtype=LD)
            np.add.at(y, (b, r), c.feat.astype(LD) * vec.astype(LD)[b, s])
            _agrees(C.restated(name, "spmv", transpose), y, (name, "spmv", transpose))
            assert np.array_equal(C.restated(name, "edge", transpose).value, g.astype(np.float64)[b, r] * vec.astype(np.float64)[b, s])
            for ncols in c.widths:
                panel, gp = C.panels(name, ncols)
                Y = np.zeros((c.batch, c.dof, ncols), dtype=LD)
                np.add.at(Y, (b, r), c.feat.astype(LD)[:, None] * panel.astype(LD)[b, s])
                _agrees(C.restated(name, "spmm", transpose, ncols), Y, (name, "spmm", ncols, transpose))
                _agrees(C.restated(name, "sddmm", transpose, ncols), (gp.astype(LD)[b, r] * panel.astype(LD)[b, s]).sum(axis=1),
                        (name, "sddmm", ncols, transpose))


def test_restated_guards():
    """the range guard: the outputs of out_of_range are those of its valid triples alone, bit for bit, and edge / sddmm give exactly 0.0
    for the others.  The zero guard: spmm is finite on explicit_zeros and equal to the result without the zero triples; spmv has no
    such guard and carries IEEE's 0 * inf = NaN to exactly the rows the zero triples write."""
    c = C.case("out_of_range")
    ok, valid = C.valid_part(c)
    assert (~ok).sum() == 8 and not ok[0] and not ok[-1] and np.any(~ok[1:-1])
    vec, g = C.vectors(c.name)
    for t in C.TRANSPOSES:
        assert np.array_equal(C.restated(c.name, "spmv", t).value, R.spmv(valid.idx, valid.feat, vec, c.batch, c.dof, t).value)
        e = C.restated(c.name, "edge", t)
        assert np.all(e.value[~ok] == 0.0) and np.all(e.m[~ok] == 0) and np.all(e.value[ok] != 0.0)
        for ncols in c.widths:
            panel, gp = C.panels(c.name, ncols)
            assert np.array_equal(C.restated(c.name, "spmm", t, ncols).value,
                                  R.spmm(valid.idx, valid.feat, panel, c.batch, c.dof, ncols, t).value)
            d = C.restated(c.name, "sddmm", t, ncols)
            assert np.all(d.value[~ok] == 0.0) and np.all(d.m[~ok] == 0) and np.all(d.value[ok] != 0.0)
    z = C.case("explicit_zeros")
    zero = z.feat == 0.0
    assert zero.sum() == 8 and np.any(np.signbit(z.feat[zero])) and not np.all(np.signbit(z.feat[zero]))
    vec, _ = C.vectors(z.name)
    assert not np.isfinite(vec[:, list(z.poisoned)]).any() and np.isfinite(np.delete(vec, z.poisoned, axis=1)).all()
    for t in C.TRANSPOSES:
        row, col = (2, 1) if t else (1, 2)
        y = C.restated(z.name, "spmv", t).value
        hit = np.zeros_like(y, dtype=bool)
        poisoned_read = zero & np.isin(z.idx[:, col], z.poisoned)
        hit[z.idx[poisoned_read, 0], z.idx[poisoned_read, row]] = True
        assert hit.any() and np.array_equal(np.isnan(y), hit) and np.isfinite(y[~hit]).all()
        for ncols in z.widths:
            panel, _ = C.panels(z.name, ncols)
            Y = C.restated(z.name, "spmm", t, ncols)
            assert np.isfinite(Y.value).all()
            assert np.array_equal(Y.value, R.spmm(z.idx[~zero], z.feat[~zero], panel, z.batch, z.dof, ncols, t).value)
            assert np.all(Y.value[:, list(z.poisoned)] == 0.0)
            assert not np.isfinite(C.restated(z.name, "sddmm", t, ncols).value[poisoned_read]).any()     # sddmm reads no feature


@pytest.mark.parametrize("name", C.INTEGER_COO_CASES)
def test_coo_restatement_matches_scipy_on_integer_values(name):
    rows, cols, vals, n = C.coo_case(name)
    assert np.array_equal(vals, np.round(vals))
    ref = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    ref.sum_duplicates()
    ref.sort_indices()
    rowptr, col, val = C.coo_restated(name)
    assert np.array_equal(rowptr, ref.indptr) and np.array_equal(col, ref.indices) and np.array_equal(val, ref.data)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float64


@pytest.mark.parametrize("name", C.STORAGE_ORDER_COO_CASES + ("nnz1",))
def test_coo_restatement_matches_a_loop_over_the_keys(name):
    rows, cols, vals, n = C.coo_case(name)
    sums = {}
    for r, s, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):             # front to back: storage order
        sums[(r, s)] = sums[(r, s)] + v if (r, s) in sums else v
    keys = sorted(sums)
    rowptr, col, val = C.coo_restated(name)
    assert col.tolist() == [k[1] for k in keys] and val.tolist() == [sums[k] for k in keys]
    assert rowptr.tolist() == [sum(1 for k in keys if k[0] < i) for i in range(n + 1)]


# ---- 2. every case reaches what it claims -----------------------------------------------------------------------------------------------
def test_shape_facts():
    c = C.case("stride_spmv")
    assert (C.SPMV_CAP, C.EDGE_CAP, C.SPMM_CAP, C.SDDMM_CAP) == (4096 * 256, 4096 * 256, 16384 * 256, 32768)
    assert c.nnz == C.SPMV_CAP + 257 > C.SPMV_CAP and c.nnz % C.BLOCK == 1 and (c.batch, c.dof) == (2, 4096)
    assert C.first_duplicate(c) > 0 and 100 < c.nnz / (c.batch * c.dof) < 160
    e = C.case("stride_edge")
    assert e.nnz == C.EDGE_CAP + 257 > C.EDGE_CAP and (e.batch, e.dof) == (2, 4096)
    d = C.case("stride_sddmm")
    assert d.nnz == C.SDDMM_CAP + 5 > C.SDDMM_CAP and d.widths == (3,) and d.dof == 512
    m = C.case("stride_spmm")
    assert m.nnz == 65537 and m.widths == (65,) and m.dof == 2048 and m.nnz * 65 > C.SPMM_CAP and "stride_spmm" in C.GRAD_CASES
    assert m.nnz > C.SDDMM_CAP                          # its feature gradient strides in sddmm as well
    w = C.case("widths")
    assert w.widths == (1, 2, 63, 64, 65, 128, 130) and (w.batch, w.dof) == (3, 37) and C.first_duplicate(w) > 0
    b = C.case("batch_offsets")
    per_sample = np.bincount(b.idx[:, 0], minlength=b.batch)
    assert b.batch == 5 and per_sample[0] == 0 and per_sample[3] == 0 and per_sample[2] == 1 and per_sample[1] > 1 and per_sample[4] > 1
    assert b.idx[b.idx[:, 0] == 2].tolist() == [[2, b.dof - 1, 0]]
    cells = {tuple(t) for t in b.idx.tolist()}
    assert sum((s, j, i) not in cells for s, i, j in cells) > len(cells) // 2      # far from symmetric
    a = C.case("all_duplicates")
    assert a.nnz == 300 and len(np.unique(a.idx, axis=0)) == 1
    z = C.case("empty")
    assert z.nnz == 0 and z.idx.shape == (0, 3)
    for name in C.CASES:
        c = C.case(name)
        assert c.idx.dtype == np.int32 and c.feat.dtype == np.float32 and c.idx.shape == (c.nnz, 3)
        finite = c.feat[c.feat != 0]
        assert np.all((np.abs(finite) >= 0.5) & (np.abs(finite) <= 2.0))
        for x in C.vectors(name) + tuple(p for w_ in c.widths for p in C.panels(name, w_)):
            assert x.dtype == np.float32 and np.all((np.abs(x[np.isfinite(x)]) >= 0.5) & (np.abs(x[np.isfinite(x)]) <= 2.0))
    # COO -> CSR
    rows, cols, vals, n = C.coo_case("storage_order")
    _, counts = np.unique(rows * n + cols, return_counts=True)
    assert 2000 < len(rows) < 5000 and sorted(set(counts.tolist())) == [1, 2, 7, 64] and not np.array_equal(vals, np.round(vals / 2) * 2)
    assert C.coo_case("n1")[3] == 1 and len(C.coo_case("nnz1")[0]) == 1
    for n_, name in ((256, "n256"), (257, "n257")):
        rows, cols, _, n = C.coo_case(name)
        assert n == n_ and rows.max() == n - 1 and cols.max() == n - 1 and rows.min() == 0
    rows, cols, _, n = C.coo_case("one_run")
    assert len(rows) == 5000 and len(set(zip(rows.tolist(), cols.tolist()))) == 1
    rows, cols, _, n = C.coo_case("sorted")
    key = rows * n + cols
    assert np.all(np.diff(key) >= 0) and np.any(np.diff(key) == 0)
    rows, cols, _, n = C.coo_case("reverse_sorted")
    key = rows * n + cols
    assert np.all(np.diff(key) <= 0) and np.any(np.diff(key) == 0)


# ---- 3. the tolerance condition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_the_bound_lies_below_a_quarter_of_the_smallest_term(name):
    """gamma_m S < min |term| / 4 for every finite output of every operator, transpose, width and gradient the GPU tests compare"""
    worst = 0.0
    for label, res in C.every_restated(name):
        finite = np.isfinite(res.value) & (res.m > 0)
        if not finite.any():
            continue
        ratio = res.bound()[finite] / res.smallest[finite]
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio < 0.25), (label, float(ratio.max()), int(res.m.max()))
        assert np.all(res.bound()[res.m == 0] == 0.0)           # an output nothing contributes to has to be exactly 0
    print(f"{name}: largest bound / smallest term = {worst:.3g}")


# ---- 4. mutants ---------------------------------------------------------------------------------------------------------------------------
# mutant -> the (case, operator, width) on which it has to show; the distances of every case are in profiles/coo_edges.md
NAMED = {
    C.MUTANTS[0]: [("batch_offsets", op, w) for op, w in (("spmv", 0), ("edge", 0), ("spmm", 5), ("sddmm", 5))],
    C.MUTANTS[1]: [("batch_offsets", op, w) for op, w in (("spmv", 0), ("edge", 0), ("spmm", 5), ("sddmm", 5))],
    C.MUTANTS[2]: [("stride_spmv", "spmv", 0), ("stride_edge", "edge", 0), ("stride_sddmm", "sddmm", 3), ("stride_spmm", "spmm", 65)],
    C.MUTANTS[3]: [("all_duplicates", op, w) for op, w in (("spmv", 0), ("edge", 0), ("spmm", 3), ("sddmm", 3))] + [("widths", "spmm", 64)],
    C.MUTANTS[4]: [("widths", op, w) for op in ("spmm", "sddmm") for w in (65, 128, 130)],
}


@pytest.mark.parametrize("which", C.MUTANTS)
def test_a_mutant_of_the_restatement_lies_far_outside_the_bound(which):
    for name, op, ncols in NAMED[which]:
        for transpose in C.TRANSPOSES:
            other = C.mutated(name, op, transpose, ncols, which)
            assert other is not None, (name, op)
            far = C.distance(C.restated(name, op, transpose, ncols), other)
            print(f"{which}: {name} {op}[{ncols}] transpose={int(transpose)}: {far:.3g} bounds away")
            assert far >= 10.0, (which, name, op, ncols, transpose, far)


def test_columns_below_64_do_not_show_the_column_mutant():
    """the boundary is AT 64: widths up to 64 are untouched by it, so 63 / 64 / 65 bracket it"""
    for ncols in (1, 2, 63, 64):
        assert C.mutated("widths", "spmm", False, ncols, C.MUTANTS[4]) is None


@pytest.mark.parametrize("name", C.STORAGE_ORDER_COO_CASES)
def test_an_unstable_sort_changes_the_sums(name):
    """COO -> CSR is held to the restatement bit for bit, so any difference shows; integer values would hide this one"""
    stable, unstable = C.coo_restated(name), C.coo_restated(name, stable=False)
    assert np.array_equal(stable[0], unstable[0]) and np.array_equal(stable[1], unstable[1])
    differ = stable[2] != unstable[2]
    print(f"{name}: {int(differ.sum())} of {len(differ)} sums differ, by up to {np.abs(stable[2] - unstable[2]).max():.3g}")
    assert differ.any()
    if name == "storage_order":
        rows, cols, _, n = C.coo_case(name)
        _, inverse, counts = np.unique(rows * n + cols, return_inverse=True, return_counts=True)
        assert set(counts[differ].tolist()) == {7, 64}          # runs of 1 and 2 have one order; every longer length shows it
    for integer in C.INTEGER_COO_CASES[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(C.coo_restated(integer), C.coo_restated(integer, stable=False)))
