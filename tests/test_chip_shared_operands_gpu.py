"""The whole-chip solve's product q = A p where a wave takes the operands it holds itself -- the own rows' p and those of the rows beside
them -- from its registers instead of gathering them (dpcg_chip.hip: rows stored around a centre, one bit per wave and slot-row).

Every case requires count, status, history and x to agree BIT FOR BIT: the default run, the runs with DPCG_CHIP_SHARED=0 (the packed
instantiation: every operand gathered) and =1 (the centred one whatever the matrix), and the CPU restatement with the chip kernel's reduction tree.  Every case also asserts how many (wave,
slot-row) pairs took the new path, against a count made here from the matrix alone (`_pairs`), so that no case passes by never taking it.
(Every system has more than 65 536 rows, which is what a plain call hands to the chip kernel; DPCG_CHIP_MIN_ROWS is read once per process
and is not needed.)  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

WAVE, THREADS, WGS = 64, 512, 256


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()  # raises if the HIP extension is missing: no silent fallback
    return pkg


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(A):
    """CSR parts exactly as stored (a scipy matrix handed over as such would be put into canonical order first)."""
    return (np.asarray(A.indptr, dtype=np.int32), np.asarray(A.indices, dtype=np.int32), np.asarray(A.data, dtype=np.float64))


def _centred_rows(A, wmax):
    """Per row: its entries, in stored order, read A.., [row - 1], row, [row + 1], B.. with at most wmax // 2 - 1 of A and
    wmax - wmax // 2 - 2 of B (the first entry on the diagonal is the centre)."""
    n = A.shape[0]
    rp, ci = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    js = wmax // 2
    lens = np.diff(rp)
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(ci.size) - rp[rows]
    on_diag = ci == rows
    jd = np.full(n, 1 << 20)
    np.minimum.at(jd, rows[on_diag], pos[on_diag])
    found = jd < (1 << 20)
    jd = np.where(found, jd, 0)
    here = rp[:-1] + jd
    has_l = found & (jd >= 1) & (ci[np.maximum(here - 1, 0)] == np.arange(n) - 1)
    has_r = found & (jd + 1 < lens) & (ci[np.minimum(here + 1, ci.size - 1)] == np.arange(n) + 1)
    return found & (jd - has_l <= js - 1) & (lens - jd - 1 - has_r <= wmax - js - 2)


def _pairs(A, per):
    """((wave, slot-row) pairs on the centred path, pairs with a row at all) as the kernel's geometry has them: workgroup v owns rows
    [v per, (v + 1) per), its thread t row v per + t + 512 k, so a pair holds up to 64 consecutive rows; it is centred when all its rows
    are and it has more than one.  A matrix with a column 32 768 or more from its row is streamed: no pairs."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    if np.abs(A.indices.astype(np.int64) - rows).max() > 32767:
        return 0, 0
    wmax = 5 if np.diff(A.indptr).max() <= 5 else (7 if np.diff(A.indptr).max() <= 7 else 9)
    ok = _centred_rows(A, wmax)
    centred = total = 0
    for v in range(WGS):
        lo, hi = v * per, min((v + 1) * per, n)
        for first in range(lo, hi, WAVE):            # (512 k + 64 w + lane runs through the workgroup's rows in order)
            last = min(first + WAVE, hi)
            total += 1
            centred += int(last - first > 1 and ok[first:last].all())
    return centred, total


def _check(D, monkeypatch, A, b, *, kind="jacobi", x0=None, flags=0, max_iter=1024, expect=None):
    """The comparison: the default run, DPCG_CHIP_SHARED=0, =1 and the CPU restatement; returns (default result, (centred pairs, pairs)).
    expect: a predicate on (centred, total).  The library takes the instantiation with the centred path by itself where at least 62 % of
    the pairs are centred (dpcg_solve_chip.hip); =1 takes it whatever the matrix, so the path's count is asserted for every matrix."""
    n = A.shape[0]
    S = D.CsrSystem.from_any(_raw(A), reorder=None)
    S.set_preconditioner(D.Jacobi() if kind == "jacobi" else None)
    ci = S.chip_info()
    assert ci["chip_by_default"], ci
    want = _pairs(A, ci["rows_per_workgroup"])
    if expect is not None:
        assert expect(*want), want
    by_default = want if 50 * want[0] >= 31 * want[1] else (0, want[1])
    db, dx0 = _dev(b), None if x0 is None else _dev(x0)
    runs = []
    for env, count in ((None, by_default), ("0", (0, want[1])), ("1", want)):
        if env is None:
            monkeypatch.delenv("DPCG_CHIP_SHARED", raising=False)
        else:
            monkeypatch.setenv("DPCG_CHIP_SHARED", env)
        r = S.solve(db, dx0, flags=flags, max_iter=max_iter)
        got = S.chip_info()
        print(f"n={n} per={ci['rows_per_workgroup']} DPCG_CHIP_SHARED={env}: {got['shared_pairs']} of {got['pairs']} pairs centred (expected {count}), {r.iterations} updates")
        assert (got["shared_pairs"], got["pairs"]) == count, env
        runs.append((f"DPCG_CHIP_SHARED={env}", r))
    monkeypatch.delenv("DPCG_CHIP_SHARED")
    res = runs[0][1]
    tree = {**S.reduction_geometry(), "form": "chip", "rows_per_workgroup": ci["rows_per_workgroup"]}
    _, it, hist, x = CO.pcg(A, b, kind, dinv=O.jacobi_dinv(A) if kind == "jacobi" else None, x0=x0, max_iter=max_iter,
                            mixed=bool(flags & D._lib.SPMV_F32), device_tree=tree)
    for name, r in runs:
        assert r.iterations == it and r.status == res.status, (name, r.iterations, it, r.status)
        assert np.array_equal(r.res_history, hist), (name, int(np.argmax(r.res_history != hist)))
        assert np.array_equal(r.x.cpu().numpy(), x), name
    assert res.iterations > 0
    S.close()
    return res, want


def _grid2d(nx, ny):
    """5-point Laplacian on an nx x ny grid, x the fast index: row i = iy nx + ix, columns ascending."""
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    A = (sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx))).tocsr()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


@pytest.fixture(scope="module")
def A41():
    return O.poisson3d(41)


mostly_centred = lambda c, t: 2 * c > t


@pytest.mark.parametrize("kind", ["jacobi", "none"])
def test_poisson3d_41(D, monkeypatch, A41, kind):
    """68 921 rows, 270 a workgroup: four full waves, one with 14 rows, three without any (and 71 rows in the last workgroup)."""
    _check(D, monkeypatch, A41, O.rhs(A41.shape[0], 0), kind=kind, expect=mostly_centred)


def test_poisson2d_257(D, monkeypatch):
    """Rows of five entries (WMAX 5: the centre in slot 2, one slot on either side of the three shared ones)."""
    A = O.poisson2d(257)
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=mostly_centred)


def test_grid_64_by_1030(D, monkeypatch):
    """x the fast index and 64 wide: where a wave starts on a grid line, lane 0 has no row - 1 entry and lane 63 no row + 1 entry (the edge
    gather asks for nothing); elsewhere the grid line ends inside the wave."""
    A = _grid2d(64, 1030)
    assert A.shape[0] == 65920
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=mostly_centred)


def test_poisson3d_81_eight_rows_a_thread(D, monkeypatch):
    """531 441 rows: eight rows a thread, seven entries a row -- the instantiation of the headline system."""
    A = O.poisson3d(81)
    res, _ = _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), max_iter=30, expect=mostly_centred)
    assert res.iterations == 30 and (A.shape[0] + WGS - 1) // WGS > 4 * THREADS


def _descending(A, rows):
    """A with the entries of `rows` stored in descending column order (not centred: the diagonal's neighbours change sides)."""
    A = A.copy()
    for i in rows:
        s, e = A.indptr[i], A.indptr[i + 1]
        A.indices[s:e] = A.indices[s:e][::-1].copy()
        A.data[s:e] = A.data[s:e][::-1].copy()
    return A


def test_mixed_waves_scattered(D, monkeypatch, A41):
    """2 000 rows, chosen by seed, stored in descending column order: their waves gather everything, the others do not.  Four pairs in five
    hold such a row, so by itself the library takes the packed instantiation here; DPCG_CHIP_SHARED=1 takes the other one."""
    A = _descending(A41, np.random.default_rng(7).choice(A41.shape[0], 2000, replace=False))
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=lambda c, t: 0 < 50 * c < 31 * t)


def test_mixed_waves_in_runs(D, monkeypatch, A41):
    """40 runs of 64 rows, their starts chosen by seed (2 560 rows): few pairs hold such a row, the default run takes the centred path for
    the others."""
    starts = np.random.default_rng(7).choice(A41.shape[0] - 64, 40, replace=False)
    A = _descending(A41, np.unique(np.concatenate([np.arange(s0, s0 + 64) for s0 in starts])))
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=lambda c, t: 31 * t <= 50 * c < 50 * t)


def test_no_row_centred(D, monkeypatch, A41):
    """EVERY row in descending order, resident: no pair is centred -- the packed instantiation by default, and under DPCG_CHIP_SHARED=1 the
    other one with every slot-row on its packed path (the per-row byte of `lens` then holds a length)."""
    A = _descending(A41, np.arange(A41.shape[0]))
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=lambda c, t: c == 0 and t > 0)


def _nine_point(n):
    """9-point stencil on an n x n grid (8 on the diagonal, -1 to the eight neighbours; weakly diagonally dominant, SPD), columns ascending:
    three entries on either side of row - 1, row, row + 1."""
    T = sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1])
    A = (9.0 * sp.identity(n * n) - sp.kron(T, T)).tocsr()
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def test_nine_point_rows(D, monkeypatch):
    """Rows of nine entries (WMAX 9: the centre in slot 4, three slots on either side -- the two-bit counts at their limit)."""
    A = _nine_point(257)
    assert np.diff(A.indptr).max() == 9 and A.diagonal().min() == 8.0
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=mostly_centred)


def test_unstructured_like(D, monkeypatch, A41):
    """A scattered numbering: no row has its neighbours beside it, and columns lie further from their rows than the resident form
    reaches -- the streamed form, which has no such path: no pairs, the same results."""
    A = O.unstructured_like(A41, seed=1)
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), expect=lambda c, t: c == 0)


@pytest.mark.parametrize("dim", [3, 2])
def test_start_vector(D, monkeypatch, A41, dim):
    """r = b - A x0 runs through the same product while the granules hold {x0, 0}: the shared operands are x0 of the own rows."""
    A = A41 if dim == 3 else O.poisson2d(257)
    _check(D, monkeypatch, A, O.rhs(A.shape[0], 0), x0=O.rhs(A.shape[0], 5), expect=mostly_centred)


def test_spmv_f32(D, monkeypatch, A41):
    """DPCG_SPMV_F32 (MODE 4): an operand from a register is rounded to fp32 as a gathered one is."""
    _check(D, monkeypatch, A41, O.rhs(A41.shape[0], 0), flags=D._lib.SPMV_F32, expect=mostly_centred)


def test_signed_zeros(D, monkeypatch, A41):
    """z_0 = -0.0 in a run of rows across a wave edge, +0.0 in another: in the first update a register holds -0.0 where the granule gives
    -0.0 + 0 * 0 = +0.0 -- the sign of a zero product, which no sum can tell."""
    b = O.rhs(A41.shape[0], 0)
    b[40:90] = -0.0
    b[100:150] = 0.0
    assert np.signbit(b[40:90]).all() and not np.signbit(b[100:150]).any()
    res, _ = _check(D, monkeypatch, A41, b, expect=mostly_centred)
    assert len(res.res_history) > 3


def test_stored_zero_beside_the_diagonal(D, monkeypatch, A41):
    """A stored 0.0 in the row + 1 place (and its mirror image) of every seventh row is an ENTRY, not a hole: the rows stay centred."""
    A = A41.copy()
    n = A.shape[0]
    hit = 0
    for i in range(3, n - 1, 7):
        s, e = A.indptr[i], A.indptr[i + 1]
        at = np.flatnonzero(A.indices[s:e] == i + 1)
        if at.size == 0:
            continue
        A.data[s + at[0]] = 0.0
        s2, e2 = A.indptr[i + 1], A.indptr[i + 2]
        A.data[s2 + np.flatnonzero(A.indices[s2:e2] == i)[0]] = 0.0
        hit += 1
    assert hit > 9000 and A.nnz == A41.nnz
    _check(D, monkeypatch, A, O.rhs(n, 0), expect=mostly_centred)


def test_one_handle_three_runs(D, monkeypatch, A41):
    """default, DPCG_CHIP_SHARED=0, default on ONE handle: nothing of a run stays behind."""
    b = _dev(O.rhs(A41.shape[0], 0))
    S = D.CsrSystem.from_any(_raw(A41), reorder=None)
    S.set_preconditioner(D.Jacobi())
    want = _pairs(A41, S.chip_info()["rows_per_workgroup"])
    runs = []
    for env in (None, "0", None):
        if env is None:
            monkeypatch.delenv("DPCG_CHIP_SHARED", raising=False)
        else:
            monkeypatch.setenv("DPCG_CHIP_SHARED", env)
        runs.append(S.solve(b))
        got = S.chip_info()
        assert (got["shared_pairs"], got["pairs"]) == ((0 if env else want[0]), want[1]) and want[0] > 0
    for r in runs[1:]:
        assert r.iterations == runs[0].iterations and np.array_equal(r.res_history, runs[0].res_history) and torch.equal(r.x, runs[0].x)
    S.close()
