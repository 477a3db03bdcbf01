"""What tests/test_bicgstab_edges_gpu.py relies on, asserted on the CPU: conditions on the inputs of bicgstab_edge_cases.py.

  every short-run pair: the restatement's history and x move by <= 1e-12 between np.sum(a * b) and a 256-way strided sum at the K the
  device test uses (`pytest -s` prints each; worst measured 8.0e-13, 13pt_24x24_pe20 under Jacobi; 725x725_pe3: 8.2e-16 / 5.3e-16);
  the shapes are what the device code paths need (odd n, pairs and lanes of the forced grids, workgroup counts, row lengths);
  every breakdown input breaks where the table says, derived twice: by the restatement under both summation orders and by the
  recurrence's scalars in rational arithmetic, which also shows that every float the recurrence meets is exact.
"""

from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_cases as C
import bicgstab_edge_cases as E
import bicgstab_restatement as R

SPREAD = 1e-12
KBLOCK, KMAXGRID, KSTREAMROWS, KTILEMINBLOCKS = 256, 1024, 256, 1536      # dpcg_internal.h


@pytest.mark.parametrize("name,pre", E.SHORT_PAIRS)
def test_the_short_runs_keep_the_spread(name, pre):
    k = E.K_OF[(name, pre)]
    hs, xs = E.short_spread(name, pre, k)
    ref = E.restated(name, pre, k)
    print(f"{name} {pre}: K = {k}, history spread {hs:.2e}, x spread {xs:.2e}, status {ref['status']} after {ref['iterations']} updates")
    assert hs <= SPREAD and xs <= SPREAD
    if (name, pre) in E.STOPS_INSIDE:
        for out in (ref, E.restated(name, pre, k, True)):
            assert out["status"] == R.OK and out["iterations"] == E.STOPS_INSIDE[(name, pre)] < k
            h = out["history"]
            assert h[-2] >= C.MARGIN * E.RTOL_SQ and C.MARGIN * h[-1] <= E.RTOL_SQ
    else:
        assert ref["status"] == R.MAX_ITER and ref["iterations"] == k == E.restated(name, pre, k, True)["iterations"]
    if k < E.K:                                            # a lowered K is the largest that holds
        assert max(E.short_spread(name, pre, k + 1)) > SPREAD


@pytest.mark.parametrize("grid", E.CHILD)
def test_the_child_process_runs_keep_the_spread_and_have_the_trips(grid):
    name, pairs, lanes, trips = E.CHILD[grid]
    n = E.matrix(name).shape[0]
    assert n % 2 == 1 and n // 2 == pairs and lanes == grid * KBLOCK and -(-pairs // lanes) == trips >= 2
    assert pairs % lanes != 0, "the last trip is ragged"
    for pre in C.PRECONDS:
        hs, xs = E.short_spread(name, pre, E.K)
        print(f"{name} {pre}: history spread {hs:.2e}, x spread {xs:.2e}")
        assert hs <= SPREAD and xs <= SPREAD and E.restated(name, pre)["iterations"] == E.K
    hs, xs = E.short_spread(name, E.CHILD_X0_PRE, E.K, x0=True)
    print(f"{name} {E.CHILD_X0_PRE} from x0: history spread {hs:.2e}, x spread {xs:.2e}")
    assert hs <= SPREAD and xs <= SPREAD and E.restated(name, E.CHILD_X0_PRE, x0=True)["iterations"] == E.K


def test_the_natural_sizes_are_what_the_passes_need():
    n257, n725 = E.matrix("257x257_pe3").shape[0], E.matrix("725x725_pe3").shape[0]
    assert n257 == 66049 and -(-n257 // KBLOCK) == 259 == E.VEC_GRID["257x257_pe3"] > KBLOCK
    assert n725 == 525625 and n725 % 2 == 1 and -(-n725 // KBLOCK) > KMAXGRID == E.VEC_GRID["725x725_pe3"]
    assert n725 // 2 - KMAXGRID * KBLOCK == 668, "lanes that take a second 16-byte trip"
    assert -(-n725 // KSTREAMROWS) >= KTILEMINBLOCKS, "the tile plan is considered by default"


def test_the_systems_made_here_are_nonsymmetric_and_have_the_rows_the_plans_need():
    B = E.matrix("13pt_24x24_pe20")
    assert B.has_sorted_indices and B.getnnz(axis=1).max() == 13 and abs(B - B.T).max() > 1.0
    assert 8 < B.nnz / B.shape[0] <= 16                                  # make_plan: 8 lanes a row
    Rg = E.matrix("ragged_2001")
    lens = Rg.getnnz(axis=1)
    assert Rg.shape[0] % 2 == 1 and lens.min() == 1 and lens.max() == 40 and set(lens) == set(range(1, 41))
    assert 16 < Rg.nnz / Rg.shape[0] <= 32                               # 16 lanes a row
    off = Rg - sp.diags(Rg.diagonal())
    assert np.all(Rg.diagonal() >= np.asarray(abs(off).sum(axis=1)).ravel() + 0.049) and abs(off).max() < 1.0
    assert ((off != 0) != (off != 0).T).nnz > 0 and abs(Rg - Rg.T).max() > 0.5, "neither pattern nor values are mirrored"
    for name in ("13pt_24x24_pe20", "ragged_2001"):                       # more entries in a 256-row block than the stream kernel's buffer holds
        A = E.matrix(name)
        assert max(A.indptr[min(i + 256, A.shape[0])] - A.indptr[i] for i in range(0, A.shape[0], 256)) > 2047
    Mx = E.matrix(E.MIX)
    offm = Mx - sp.diags(Mx.diagonal())
    assert Mx.shape[0] == E.MIX_SIDE ** 2 and abs(Mx - Mx.T).max() > 0.02
    assert np.all(Mx.diagonal() >= np.asarray(abs(offm).sum(axis=1)).ravel() - 1e-12), "row dominant"
    up, lo = sp.triu(Mx, 1).tocsr(), sp.tril(Mx, -1).T.tocsr()
    assert abs(up - 0.9 * lo).max() < 1e-15, "the upper triangle is 0.9 x the mirrored lower one"
    a20, a5 = E.matrix(E.LIFE_SYSTEM), E.matrix(E.NEW_VALUES)
    assert np.array_equal(a20.indptr, a5.indptr) and np.array_equal(a20.indices, a5.indices) and not np.array_equal(a20.data, a5.data)


@pytest.mark.parametrize("name", E.BREAKDOWNS)
def test_every_breakdown_input_breaks_where_the_table_says(name):
    A, b, what, status, updates, history, x = E.BREAKDOWNS[name]
    for copies in (1, E.KRON):
        Ak, bk = E.breakdown_csr(name, copies)
        assert Ak.nnz == copies * b.size ** 2, "every entry is stored, zeros too"
        assert np.array_equal(Ak.toarray(), np.kron(np.eye(copies), A)) if copies == 1 else Ak.shape[0] == copies * b.size
        for dot in (R.plain_dot, R.strided_dot):
            for max_iter in (2, 1024):
                ref = R.bicgstab(Ak, bk, max_iter=max_iter, dot=dot)
                assert ref["status"] == status == R.BREAKDOWN and ref["iterations"] == updates
                assert ref["history"].tolist() == history and np.array_equal(ref["x"], np.tile(x, copies))
    # which statement breaks: the recurrence's scalars in rational arithmetic
    recs = E.exact_scalars(A, b, 2)
    assert len(recs) == updates + 1
    last = recs[-1]
    if what == "rv":
        assert last["rho"] != 0 and last["v_nonzero"] and last["rv"] == 0 and "alpha" not in last
    elif what == "tt":
        assert last["rho"] != 0 and last["rv"] != 0 and last["alpha"] == 1 and last["s_nonzero"] and last["tt"] == 0
    else:
        assert list(last) == ["rho"] and last["rho"] == 0, "<rhat,r> = 0 at the head of the update after a completed one"
        assert recs[0]["omega"] == (0 if name == "pass_p_rho_omega_0" else Fraction(1, 2))
    # ... and every one of them a dyadic rational of a few bits: fp64 holds them, so no summation order can change a bit
    for rec in recs:
        for key, v in rec.items():
            if isinstance(v, Fraction):
                assert v.denominator & (v.denominator - 1) == 0 and v.denominator <= 4 and abs(v.numerator) <= 16, (key, v)


def test_the_three_row_case_is_needed():
    """On two rows <rhat,r> = 0 after a completed update happens with omega = 0 only (a search over the entries -2 .. 2 and six b finds
    no other), and there a pass P WITHOUT the test gives the same answer: beta = (0 / rho)(alpha / 0) is a NaN, p and v are NaN, and
    <rhat,v> is refused by pass S -- BREAKDOWN after the same single update.  The three-row case has omega = 1/2: without the test
    beta = 0, p = r, and the update completes."""
    A, b = E.BREAKDOWNS["pass_p_rho"][:2]
    r = np.array([0.0, 0.0, 0.5])                          # after update 0 (the table's history[1] = <r,r> = 1/4)
    assert R.bicgstab(A, b)["history"].tolist() == [1.0, float(r @ r)] and float(b @ r) == 0.0
    v = A @ r                                              # beta = 0: p = r
    assert float(b @ v) != 0.0, "pass S would not stop a pass P that went on"
    t = A @ r                                              # alpha = 0 / <rhat,v> = 0: s = r
    assert float(t @ t) != 0.0, "nor would pass X"
    with np.errstate(all="ignore"):
        assert np.isnan((np.float64(0.0) / np.float64(1.0)) * (np.float64(-0.5) / np.float64(0.0)))


def test_nonfinite_and_zero_right_hand_sides_and_the_half_step_exit():
    A, b = C.matrix("23x23_pe2"), C.rhs("23x23_pe2").copy()
    x0 = E.x0_of("23x23_pe2")
    b[7] = np.inf
    for start in (None, x0):
        out = R.bicgstab(A, b, x0=start, rtol_sq=E.RTOL_SQ)
        assert out["status"] == R.BREAKDOWN and out["iterations"] == 0 and len(out["history"]) == 1 and np.isnan(out["history"][0])
        assert np.array_equal(out["x"], np.zeros_like(b) if start is None else start)
    zero = np.zeros(A.shape[0])
    out = R.bicgstab(A, zero, rtol_sq=E.RTOL_SQ, atol_sq=0.0)
    assert out["status"] == R.BREAKDOWN and out["iterations"] == 0 and not out["x"].any()
    out = R.bicgstab(A, zero, rtol_sq=E.RTOL_SQ, atol_sq=1e-30)
    assert out["status"] == R.OK and out["iterations"] == 0 and not out["x"].any()
    Dg, d, bd = E.half_step_system()
    assert d.size == E.HALF_N == 1025 and -(-E.HALF_N // KBLOCK) == 5
    for dot in (R.plain_dot, R.strided_dot):
        half = R.bicgstab(Dg, bd, lambda v: (1.0 / d) * v, rtol_sq=E.RTOL_SQ, dot=dot)
        print(f"half-step exit: history[1] {half['history'][1]:.3e} <= {E.HALF_BOUND:.3e}")
        assert half["status"] == R.OK and half["iterations"] == 1 and half["history"][1] <= E.HALF_BOUND
        np.testing.assert_allclose(half["x"], bd / d, rtol=1e-15)
