"""The device ICholT (dpcg_icholt.hip) at its edges, case table in tests/icholt_edge_cases.py (what each case is built for is asserted
on the CPU by tests/test_icholt_edges_host.py): the factor against oracle.icholt bit for bit on both sides of every limit of the
dispatcher, with the form, the waves and the retry that dpcg_get_icholt_info reports checked against the prediction -- a pipeline
defect that the one-wave kernel would repair shows as a retry nobody expected; every cap met and exceeded by one; ties, a candidate
on the threshold, exact zeros, values whose squares overflow or vanish, NaN and inf; rows stored in any order and without their
lower triangle; every refusal with its text and column and the previous preconditioner kept; re-attaching after new values."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import icholt_edge_cases as X
from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KNOBS = ("DPCG_ICHOLT_LDS", "DPCG_ICHOLT_REGS", "DPCG_ICHOLT_WAVES", "DPCG_ICHOLT_TRACE")
TEXT = {"colcap": "nnz + add_fill_in exceeds 64 entries at column {k}", "cand": "more than 256 candidates at column {k}",
        "rowcap": "a row of L would keep more than 64 entries (reached at column {k})", "pivot": "non-positive pivot at column {k}",
        "nodiag": "missing diagonal entry at column {k}"}


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


@pytest.fixture(scope="module")
def restated():
    """(matrix as the case stores it, the restated factor or its IcholtError) of a table case: computed once, never written to."""
    cache = {}

    def get(name):
        if name not in cache:
            c = X.CASE_BY_NAME[name]
            M = c.matrix()
            try:
                with np.errstate(all="ignore"):
                    L = O.icholt(X.as_csr(M), c.add_fill_in, c.threshold)
                L.data.setflags(write=False)
            except O.IcholtError as e:
                L = e
            cache[name] = (M, L)
        return cache[name]
    return get


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _dev(v):
    return torch.from_numpy(np.asarray(v, dtype=np.float64)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _factor(S):
    rp, ci, v = S.factor()
    return sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))


def _same_bits(P, Q):
    """Row pointers, columns and the BITS of the values (signed zeros, inf and NaN payloads included)."""
    return (np.array_equal(P.indptr, Q.indptr) and np.array_equal(P.indices, Q.indices) and np.array_equal(_bits(P.data), _bits(Q.data)))


def _expected_info(case, M):
    rp, ci, _ = X.arrays(M)
    form, waves, retry, cap = X.predict(rp, ci, case.add_fill_in, case.env)
    if case.retry is not None:                                      # the pipeline hands over: the one-wave kernel's factor
        form, waves, retry = 3, 0, case.retry
    return {"form": form, "waves": waves, "retry_column": retry, "pool_cap": cap}


def _system(D, M):
    return D.CsrSystem.from_any(X.arrays(M) if isinstance(M, tuple) else M, reorder=None)


def _jacobi_for(D, A):
    d = np.abs(A.diagonal())
    with np.errstate(all="ignore"):
        dinv = np.where(np.isfinite(1.0 / d), 1.0 / d, 1.0)         # (the diagonal may hold a NaN, an inf or no entry in these cases)
    return D.Jacobi(dinv)


# ---- factor bits, the form that produced them, refusals -----------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_factor_form_and_refusal(D, restated, monkeypatch, case):
    M, Lr = restated(case.name)
    _env(monkeypatch, case.env)
    S = _system(D, M)
    n = S.n
    r = O.rhs(n, 3)
    if case.refusal is not None:
        assert isinstance(Lr, O.IcholtError) and (Lr.kind, Lr.column) == (case.refusal, case.column)
        S.set_preconditioner(_jacobi_for(D, X.as_csr(M)))
        before = _bits(S.precond_apply(_dev(r)).cpu().numpy())
        with pytest.raises(D._lib.DpcgError) as e:
            S.set_preconditioner(D.ICholT("multiply", case.add_fill_in, case.threshold))
        want = D._lib.ERR_PIVOT if case.refusal in ("pivot", "nodiag") else D._lib.ERR_INVALID
        assert e.value.status == want, str(e.value)
        assert str(e.value).endswith("icholt: " + TEXT[case.refusal].format(k=case.column)), str(e.value)
        assert S.info()["precond"] == D._lib.PRECOND_JACOBI           # the previous preconditioner is still attached, and applies
        assert np.array_equal(_bits(S.precond_apply(_dev(r)).cpu().numpy()), before)
        with pytest.raises(D._lib.DpcgError) as e:
            S.icholt_info()
        assert e.value.status == D._lib.ERR_STATE
        S.close()
        return
    S.set_preconditioner(D.ICholT("multiply", case.add_fill_in, case.threshold))
    info = S.icholt_info()
    print(f"{case.name}: n = {n}, {info}")
    Ld = _factor(S)
    assert _same_bits(Ld, Lr), case.name
    assert sp.triu(Ld, 1).nnz == 0 and (Ld.diagonal() > 0).all()
    assert np.array_equal(Ld.indices[Ld.indptr[1:] - 1], np.arange(n))          # the diagonal last in every row
    assert info == _expected_info(case, M), (info, _expected_info(case, M))
    if case.form is not None and case.retry is None:
        assert info["form"] == case.form
    if not case.nonfinite:
        z = S.precond_apply(_dev(r)).cpu().numpy()
        np.testing.assert_allclose(z, Lr @ (Lr.T @ r), rtol=1e-12, atol=1e-13)
    S.close()


def test_each_form_boundary_pair_reports_two_forms(D, monkeypatch):
    _env(monkeypatch, {})
    for a, b in X.FORM_PAIRS:
        seen = []
        for name in (a, b):
            c = X.CASE_BY_NAME[name]
            S = _system(D, c.matrix())
            S.set_preconditioner(D.ICholT("multiply", c.add_fill_in, c.threshold))
            seen.append(S.icholt_info())
            S.close()
        assert [i["form"] for i in seen] == [X.CASE_BY_NAME[a].form, X.CASE_BY_NAME[b].form] and seen[0]["form"] != seen[1]["form"]
        assert seen[0]["retry_column"] is None and seen[1]["retry_column"] is None


def test_info_belongs_to_the_icholt_factor_only(D, monkeypatch):
    _env(monkeypatch, {})
    A = X.fill_case()
    S = D.CsrSystem.from_any(A, reorder=None)
    with pytest.raises(D._lib.DpcgError) as e:
        S.icholt_info()
    assert e.value.status == D._lib.ERR_STATE
    S.set_preconditioner(D.ICholT("solve", 2, 0.01))
    assert S.icholt_info()["form"] == 1
    for other in (D.IC0("solve"), D.LLtMultiply(O.icholt(A, 2, 0.01)), D.Jacobi(), None):
        S.set_preconditioner(other)
        with pytest.raises(D._lib.DpcgError) as e:
            S.icholt_info()
        assert e.value.status == D._lib.ERR_STATE
    S.close()


# ---- life cycle ---------------------------------------------------------------------------------------------------------------
def test_reordered_handle_factors_the_caller_s_numbering(D, monkeypatch):
    _env(monkeypatch, {})
    A = O.unstructured_like(O.poisson2d(20), seed=3)
    Lr = O.icholt(A, 2, 0.01)
    S = D.CsrSystem.from_any(A, reorder="rcm")
    assert S.info()["reordered"]
    S.set_preconditioner(D.ICholT("multiply", 2, 0.01))
    assert _same_bits(_factor(S), Lr) and S.icholt_info()["retry_column"] is None
    r = O.rhs(A.shape[0], 3)
    np.testing.assert_allclose(S.precond_apply(_dev(r)).cpu().numpy(), Lr @ (Lr.T @ r), rtol=1e-12, atol=1e-13)
    S.close()


@pytest.mark.parametrize("env", [{}, X.WORKSPACE, X.ONE_WAVE], ids=["lds", "workspace", "one_wave"])
def test_new_values_that_change_the_pattern_of_L(D, monkeypatch, env):
    _env(monkeypatch, env)
    t = X.THRESHOLD_CROSSING
    A1, A2 = X.penta(t["n"], second=t["before"]), X.penta(t["n"], second=t["after"])
    L1, L2 = O.icholt(A1, t["add_fill_in"], t["threshold"]), O.icholt(A2, t["add_fill_in"], t["threshold"])
    assert L1.nnz != L2.nnz
    S = D.CsrSystem.from_any(A1, reorder=None)
    M = D.ICholT("multiply", t["add_fill_in"], t["threshold"])
    S.set_preconditioner(M)
    assert _same_bits(_factor(S), L1)
    S.update_values(A2.data)
    S.set_preconditioner(M)
    assert _same_bits(_factor(S), L2) and S.icholt_info()["retry_column"] is None
    S.update_values(A1.data)
    S.set_preconditioner(M)
    assert _same_bits(_factor(S), L1)
    S.close()


def test_failed_attaches_leave_the_handle_as_it_was(D, monkeypatch):
    """dpcg_update_values drops the preconditioner by contract, so two sequences: (i) a refused attach on the SAME values (a count
    bound over the cap) keeps the attached factor, its info and its apply bit for bit; (ii) new, indefinite values: the factor went
    with the old values, the refused attach (DPCG_ERR_PIVOT at the restatement's column) puts nothing in its place, and the old
    values give the old factor again."""
    _env(monkeypatch, {})
    A = X.fill_case()
    n = A.shape[0]
    L1 = O.icholt(A, 2, 0.01)
    r = O.rhs(n, 1)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.ICholT("multiply", 2, 0.01))
    info, z = S.icholt_info(), _bits(S.precond_apply(_dev(r)).cpu().numpy())
    for _ in range(2):
        with pytest.raises(D._lib.DpcgError) as e:
            S.set_preconditioner(D.ICholT("multiply", 200, 0.01))
        assert e.value.status == D._lib.ERR_INVALID and str(e.value).endswith(TEXT["colcap"].format(k=0))
        assert S.info()["precond"] == D._lib.PRECOND_LLT_MULTIPLY and S.icholt_info() == info and _same_bits(_factor(S), L1)
        assert np.array_equal(_bits(S.precond_apply(_dev(r)).cpu().numpy()), z)
    bad = X.with_entries(A, {(77, 77): -1.0})
    with pytest.raises(O.IcholtError) as re:
        O.icholt(bad, 2, 0.01)
    assert re.value.kind == "pivot"
    S.update_values(bad.data)
    with pytest.raises(D._lib.DpcgError) as e:
        S.set_preconditioner(D.ICholT("multiply", 2, 0.01))
    assert e.value.status == D._lib.ERR_PIVOT and str(e.value).endswith(TEXT["pivot"].format(k=re.value.column))
    assert S.info()["precond"] == D._lib.PRECOND_NONE
    with pytest.raises(D._lib.DpcgError) as e:
        S.icholt_info()
    assert e.value.status == D._lib.ERR_STATE
    S.update_values(A.data)
    S.set_preconditioner(D.ICholT("multiply", 2, 0.01))
    assert S.icholt_info() == info and _same_bits(_factor(S), L1)
    assert np.array_equal(_bits(S.precond_apply(_dev(r)).cpu().numpy()), z)
    S.close()


@pytest.mark.parametrize("name", X.REPEAT_CASES)
def test_three_attaches_give_the_same_bits(D, restated, monkeypatch, name):
    """The pipeline's paths (mailbox against chain walk) depend on timing; its sums do not."""
    case = X.CASE_BY_NAME[name]
    M, Lr = restated(name)
    _env(monkeypatch, case.env)
    S = _system(D, M)
    for _ in range(3):
        S.set_preconditioner(D.ICholT("multiply", case.add_fill_in, case.threshold))
        assert _same_bits(_factor(S), Lr) and S.icholt_info() == _expected_info(case, M)
    S.close()


# ---- a solve through a 64-wide row ----------------------------------------------------------------------------------------------
def test_solve_through_a_64_wide_row(D, restated, monkeypatch):
    case = X.CASE_BY_NAME["wide_row64_fill0"]
    A, Lr = restated(case.name)
    _env(monkeypatch, {})
    assert np.diff(Lr.tocsc().indptr).max() == 65                    # column 0 of L: the diagonal and 64 kept entries
    b = O.rhs(A.shape[0], 1)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.ICholT("solve", case.add_fill_in, case.threshold))
    assert _same_bits(_factor(S), Lr)
    res = S.solve(_dev(b))
    _, it, hist, _ = CO.pcg(A, b, "llt_solve", L=Lr)
    assert res.status == 0 and abs(res.iterations - it) <= 1
    m = min(len(hist), len(res.res_history), 25)
    np.testing.assert_allclose(res.res_history[:m], hist[:m], rtol=1e-9)
    S.close()
