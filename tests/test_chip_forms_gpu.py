"""The four whole-chip one-launch forms -- standard (dpcg_chip.hip), single reduction (dpcg_chip_sr.hip), M = L L^T multiplied
(dpcg_chip_llt.hip), two triangular solves (dpcg_chip_trsv.hip) -- through the host path they share (dpcg_solve_chip.hip): what that path
does for every form alike and the parity tests of the single forms do not reach.  A library-reordered handle with a start vector, with and
without the history; the forms one after the other on ONE handle (they share its slots, its granule tables and the process's nonce
source); the kernel's time between HIP events.  (That `SolveResult.recurrence` follows the solve that ran, and a standard solve before and
after a single-reduction one on the same handle: tests/test_single_reduction_gpu.py.)  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMS = ("standard", "single_reduction", "llt_multiply", "triangular_solves")
HIST_RTOL = 1e-10          # a reordered handle against the oracle on P A P^T: the bar of tests/test_gpu_parity.py (x: rtol 1e-9, atol 1e-12)


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()  # raises if the HIP extension is missing: no silent fallback
    return pkg


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _permuted(A, perm):
    """P A P^T as the library iterates on it (row `new` = the caller's row perm[new]), canonical CSR."""
    B = A[perm][:, perm].tocsr()
    B.sort_indices()
    return B


def _attach(D, S, form, L=None):
    """The preconditioner that sends a plain call on S to `form`; L: the factor the L L^T form multiplies by, in S's caller's numbering."""
    if form == "llt_multiply":
        S.set_preconditioner(D.LLtMultiply(L))
    elif form == "triangular_solves":
        S.set_preconditioner(D.IC0("solve", ordering="multicolor"))
    else:
        S.set_preconditioner(D.Jacobi())
    assert S.chip_info()["chip_by_default"], (form, S.chip_info(), S.info())


def _solve(S, form, b, x0=None, **kw):
    """To convergence -- but 40 updates of the L L^T form: MULTIPLYING by an incomplete Cholesky factor (test.py:88 does so with the learned
    one) squares the condition number, and such a solve runs into any cap."""
    recurrence = "single_reduction" if form == "single_reduction" else "standard"
    capped = form == "llt_multiply"
    res = S.solve(b, x0, recurrence=recurrence, max_iter=40 if capped else 1024, **kw)
    assert res.recurrence == recurrence and res.status == (1 if capped else 0) and res.iterations > 0, (form, res.status, res.iterations)
    return res


@pytest.fixture(scope="module")
def p41(D):
    """41^3 (68 921 rows: the smallest grid all four forms take), its IC(0) factor, and every form's solve ALONE on a fresh handle
    (computed once, never modified)."""
    A = O.poisson3d(41)
    b = _dev(O.rhs(A.shape[0], 0))
    L = CO.ic0(A)
    alone = {}
    for form in FORMS:
        S = D.CsrSystem.from_any(A, reorder=None)
        _attach(D, S, form, L)
        alone[form] = _solve(S, form, b)
        launches = S.solve(b, flags=D._lib.NO_SMALL, max_iter=len(alone[form].res_history) - 1)
        assert not np.array_equal(launches.res_history, alone[form].res_history), form      # (other bits than the launches': it WAS the one-launch form)
        S.close()
    return A, b, L, alone


# smallest systems per form: standard / single reduction beyond the team kernel's 65 536 rows, L L^T beyond the one-workgroup kernel's
# 6 144, the triangular solves from 1 024; a scattered numbering so that reorder="rcm" has something to do
@pytest.mark.parametrize("form,make", [
    ("standard", lambda: O.unstructured_like(O.poisson3d(41), seed=1)),
    ("single_reduction", lambda: O.unstructured_like(O.poisson3d(41), seed=1)),
    ("llt_multiply", lambda: O.unstructured_like(O.poisson2d(79), seed=2)),            # 6 241 rows
    ("triangular_solves", lambda: O.unstructured_like(O.poisson2d(40), seed=3))])      # 1 600 rows
def test_reordered_handle_with_a_start_vector(D, form, make):
    """reorder="rcm": b and x0 are gathered into the handle's numbering and x scattered back by the shared path.  Count, history and x equal
    those of a reorder=None handle of P A P^T given P b and P x0 (the bar of the reorder tests in test_gpu_parity.py), and x is the same
    bits whether or not the history is asked for (the history copy and the scatter share one synchronisation)."""
    A = make()
    n = A.shape[0]
    b, x0 = O.rhs(n, 0), O.rhs(n, 5)
    R = D.CsrSystem.from_any(A, reorder="rcm")
    assert R.reordered
    perm = R.permutation()
    L = None
    if form == "llt_multiply":
        # the plain handle below is handed P L P^T, which has to be lower triangular as well: IC(0) of A without the entries that the
        # reordering turns upwards (any L with a positive diagonal makes M = L L^T symmetric positive definite)
        new = np.argsort(perm)
        F = CO.ic0(A).tocoo()
        keep = new[F.row] >= new[F.col]
        L = sp.csr_matrix((F.data[keep], (F.row[keep], F.col[keep])), shape=A.shape)
        L.sort_indices()
        assert L.nnz > n and sp.triu(_permuted(L, perm), 1).nnz == 0
    _attach(D, R, form, L)
    res = _solve(R, form, _dev(b), _dev(x0))
    bare = _solve(R, form, _dev(b), _dev(x0), want_history=False)
    assert len(bare.res_history) == 0 and bare.iterations == res.iterations and torch.equal(bare.x, res.x)
    N = D.CsrSystem.from_any(_permuted(A, perm), reorder=None)
    assert not N.reordered
    _attach(D, N, form, None if L is None else _permuted(L, perm))
    ref = _solve(N, form, _dev(b[perm]), _dev(x0[perm]))
    assert res.iterations == ref.iterations, (form, res.iterations, ref.iterations)
    np.testing.assert_allclose(res.res_history, ref.res_history, rtol=HIST_RTOL)
    np.testing.assert_allclose(res.x.cpu().numpy()[perm], ref.x.cpu().numpy(), rtol=1e-9, atol=1e-12)
    R.close()
    N.close()


def test_forms_one_after_the_other_on_one_handle(D, p41):
    """Every form after every other one, on ONE handle: they share its reduction slots and error flag (chip_part), its granule tables
    (chip_zp; chip_rt for the two factor forms) and the process-wide nonce that keys the granules.  Each solve equals, bit for bit, the
    form's solve alone on a fresh handle."""
    A, b, L, alone = p41
    order = [0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3, 0]
    assert {(u, v) for u, v in zip(order, order[1:])} == {(u, v) for u in range(4) for v in range(4) if u != v}     # each pair, both orders
    S = D.CsrSystem.from_any(A, reorder=None)
    for step, k in enumerate(order):
        form = FORMS[k]
        _attach(D, S, form, L)
        res = _solve(S, form, b)
        ref = alone[form]
        assert res.iterations == ref.iterations, (step, form, res.iterations, ref.iterations)
        assert np.array_equal(res.res_history, ref.res_history), (step, form, int(np.argmax(res.res_history != ref.res_history)))
        assert torch.equal(res.x, ref.x), (step, form)
    S.close()


def test_kernel_time_between_events(D, p41, monkeypatch):
    """DPCG_CHIP_EVENTS=1 (read per solve): chip_info()["kernel_ms"] is the kernel's time between HIP events on the launch stream for the
    standard, the single-reduction and the triangular-solve form -- positive, and no more than the solve's own `seconds`, whose host
    timer is started before the first event is recorded and stopped after the synchronisation behind the second.  A single-reduction
    solve with the events off reports 0."""
    A, b, L, _ = p41
    S = D.CsrSystem.from_any(A, reorder=None)
    monkeypatch.setenv("DPCG_CHIP_EVENTS", "1")
    for form in ("standard", "single_reduction", "triangular_solves"):
        _attach(D, S, form)
        res = _solve(S, form, b)
        ms = S.chip_info()["kernel_ms"]
        print(f"{form}: kernel {ms:.4f} ms, solve {res.seconds * 1e3:.4f} ms")
        assert 0.0 < ms <= res.seconds * 1e3, (form, ms, res.seconds)
    monkeypatch.delenv("DPCG_CHIP_EVENTS")
    _attach(D, S, "single_reduction")
    _solve(S, "single_reduction", b)
    assert S.chip_info()["kernel_ms"] == 0.0
    S.close()
