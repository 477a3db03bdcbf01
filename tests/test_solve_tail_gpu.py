"""The optional outputs of a solve stay optional on every form (dpcg_solve, dpcg_solve_refined through ctypes).

Every form ends in the same delivery of results (finish_one_launch / deliver_solve / deliver_results, dpcg_solve.hip); which of
iters, final_res, seconds and res_history the caller asked for decides what is copied and whether the host synchronises a second
time.  Per form, on the smallest system the host path sends there (the ones tools/solve_forms_digest.py uses): a call with every
optional out-pointer null, a call with all of them given and a call that asks for the history only must return the same status and
bit-identical x, and the two histories must agree entry for entry.  (err_history is left out: it needs x_true, an input that moves the
launch path to other kernels.)
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

MAX_ITER = 200


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def grid_laplacian(rows, width):
    """the 5-point Dirichlet Laplacian of a rows x width grid"""
    def line(d):
        return sp.diags([-np.ones(d - 1), 2.0 * np.ones(d), -np.ones(d - 1)], [-1, 0, 1], format="csr")
    A = sp.csr_matrix(sp.kron(sp.identity(rows), line(width)) + sp.kron(line(rows), sp.identity(width)))
    A.sort_indices()
    return A


def poisson3d_41():
    from oracle import oracle as O
    return O.poisson3d(41)


# form, matrix, flags, what the handle must report for a plain call to take that form
CASES = {
    "one_workgroup": (lambda: grid_laplacian(5, 7), 0, lambda S: S.reduction_geometry()["small_threads"] > 0),
    "team": (lambda: grid_laplacian(65, 64), 0, lambda S: S.reduction_geometry()["team_by_default"]),
    "whole_chip": (poisson3d_41, 0, lambda S: S.chip_info()["chip_by_default"]),
    "launch_path": (lambda: grid_laplacian(40, 40), 8, lambda S: True),          # 8: DPCG_NO_SMALL
    "refined": (lambda: grid_laplacian(40, 40), 0, lambda S: True),
}


def call(D, S, form, flags, b, want):
    """One ctypes call; want: which optional outputs to pass ("none", "all", "history").  Returns status, x, iters, history."""
    from deeppreconditioning_amd.operators import _dev_ptr, _np_ptr, _stream
    L = D._lib
    x = torch.full_like(b, float("nan"))
    hist = np.full(MAX_ITER + 1, np.nan) if want in ("all", "history") else None
    iters, outer, res, sec = C.c_int(-1), C.c_int(-1), C.c_double(), C.c_double()
    opt = (lambda p: C.byref(p)) if want == "all" else (lambda p: None)
    with torch.cuda.device(S.device):
        if form == "refined":
            outer_hist = np.full(17, np.nan) if want == "all" else None
            status = L.check(L.lib().dpcg_solve_refined(S._h, _dev_ptr(b), None, _dev_ptr(x), 1e-8, 0.0, MAX_ITER, 1e-6, 16, 0, _stream(),
                                                        opt(iters), opt(outer), opt(res), opt(sec), _np_ptr(hist), _np_ptr(outer_hist)))
        else:
            status = L.check(L.lib().dpcg_solve(S._h, _dev_ptr(b), None, _dev_ptr(x), 1e-8, 0.0, MAX_ITER, flags, _stream(),
                                                opt(iters), opt(res), opt(sec), _np_ptr(hist), None, None))
    return status, x.cpu().numpy(), iters.value, hist


@pytest.mark.parametrize("form", list(CASES))
def test_optional_outputs_stay_optional(D, form):
    make, flags, takes_form = CASES[form]
    A = make()
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    assert takes_form(S), (form, S.reduction_geometry(), S.chip_info())
    b = torch.from_numpy(np.random.default_rng(1).random(A.shape[0])).cuda()
    st_none, x_none, _, _ = call(D, S, form, flags, b, "none")
    st_all, x_all, iters, hist_all = call(D, S, form, flags, b, "all")
    st_hist, x_hist, _, hist_only = call(D, S, form, flags, b, "history")
    S.close()
    assert st_none == st_all == st_hist
    assert 0 < iters <= MAX_ITER
    assert np.isfinite(x_all).all()
    assert np.array_equal(x_none, x_all) and np.array_equal(x_hist, x_all)
    assert np.isfinite(hist_all[:iters + 1]).all()
    assert np.array_equal(hist_only[:iters + 1], hist_all[:iters + 1])
    assert np.isnan(hist_all[iters + 1:]).all() and np.isnan(hist_only[iters + 1:]).all()
