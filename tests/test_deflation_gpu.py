"""Deflated PCG on the device (dpcg_set_deflation, `CsrSystem.set_deflation`, dpcg_deflation.hip) against the numpy restatement
(tests/deflation_restatement.py).  In every case W is uploaded and the restatement is fed the A-orthonormal W and AW that
dpcg_get_deflation returns.

Shapes: 5x7 (35 rows: fewer than one workgroup, odd n, the tail element), 33x31 (1023: odd, several workgroups), 40x40, the seeded
edge-weighted 32x32 and 10x12x9 Laplacians + 0.05 I.  k = 1, 3, 8 (stored as 1, 4 and 8 columns), M = I and Jacobi.  W = the k lowest
eigenvectors of M A from a dense eigh; b = default_rng(1).random(n).

A case is a count case where the restatement's stop margin is >= 1.2 AND its history moves by less than 1e-11 relative under a 1e-16
relative perturbation of b (both evaluated here, with the device's W).  COUNT_CASES lists those the CPU classification found with
room to spare -- the test asserts both properties for them; every other case is compared by its true residual only (unpreconditioned
CG on the seeded systems is chaotic in the restatement itself, and several Jacobi cases stop within 1.1 of the threshold).
"""

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import deflation_restatement as R
import spectrum_restatement as LZ
from deeppreconditioning_amd.poisson import subdomain_indicators

pytestmark = pytest.mark.gpu

HIST_RTOL = 1e-10
RTOL_SQ = 1e-8
EPS = np.finfo(float).eps

SYSTEMS = {
    "5x7": lambda: R.poisson((5, 7)),
    "33x31": lambda: R.poisson((33, 31)),
    "40x40": lambda: R.poisson((40, 40)),
    "w32x32": lambda: R.shifted_laplacian((32, 32), 3),
    "w10x12x9": lambda: R.shifted_laplacian((10, 12, 9), 5),
}
ALL_CASES = [(name, k, pre) for name in SYSTEMS for k in (1, 3, 8) for pre in ("identity", "jacobi")]
COUNT_CASES = ([("5x7", k, pre) for k in (1, 3, 8) for pre in ("identity", "jacobi")]
               + [("40x40", k, pre) for k in (1, 3, 8) for pre in ("identity", "jacobi")]
               + [("33x31", 3, "identity"), ("33x31", 3, "jacobi"), ("w10x12x9", 8, "jacobi")])

_SYS, _EIG = {}, {}


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def system(name):
    if name not in _SYS:
        A = SYSTEMS[name]()
        _SYS[name] = (A, np.random.default_rng(1).random(A.shape[0]))
    return _SYS[name]


def eigenvectors(name, pre):
    """The 8 lowest eigenvectors of M A and all eigenvalues, computed once per (system, M)."""
    if (name, pre) not in _EIG:
        _EIG[(name, pre)] = R.low_eigenvectors(system(name)[0], 8, pre == "jacobi")
    return _EIG[(name, pre)]


def apply_of(A, pre):
    return R.jacobi(A) if pre == "jacobi" else None


def attach(D, A, W, pre, reorder=None):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.Jacobi() if pre == "jacobi" else (None if pre == "identity" else pre))
    if W is not None:
        S.set_deflation(W)
    return S


def gpu(b):
    return torch.from_numpy(np.ascontiguousarray(b)).cuda()


def hist_diff(dev, ref):
    return float(np.max(np.abs(dev - ref) / ref)) if len(dev) == len(ref) else np.inf


def stable(A, b, W, AW, m, hist):
    """The restatement's own history under a 1e-16 relative perturbation of b: the largest relative move (inf: the count moved)."""
    b2 = b + 1e-16 * np.abs(b).max() * np.random.default_rng(9).standard_normal(b.size)
    _, _, h2, _ = R.pcg(A, b2, W, AW, m, rtol_sq=RTOL_SQ)
    return hist_diff(h2, hist)


def check_orthonormal(A, W, AW):
    """|W^T A W - I|_max <= n eps max_j(|w_j|^T |A| |w_j|), the bound computed from the returned W; AW is A W to rounding."""
    n = A.shape[0]
    absA = abs(A)
    bound = n * EPS * max(float(np.abs(W[:, j]) @ (absA @ np.abs(W[:, j]))) for j in range(W.shape[1]))
    dev = np.abs(W.T @ (A @ W) - np.eye(W.shape[1])).max()
    print(f"|W^T A W - I|_max = {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound
    assert np.abs(AW - A @ W).max() <= n * EPS * np.abs(AW).max() * 8


@pytest.mark.parametrize("name,k,pre", ALL_CASES)
def test_against_the_restatement(D, name, k, pre):
    A, b = system(name)
    V, _ = eigenvectors(name, pre)
    S = attach(D, A, V[:, :k], pre)
    d = S.deflation()
    assert d["k"] == k and d["W"].shape == (A.shape[0], k)
    W, AW = d["W"], d["AW"]
    check_orthonormal(A, W, AW)
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    m = apply_of(A, pre)
    status, count, hist, x = R.pcg(A, b, W, AW, m, rtol_sq=RTOL_SQ)
    margin, moved = R.stop_margin(hist, RTOL_SQ), stable(A, b, W, AW, m, hist)
    true = R.true_residual(A, b, res.x.cpu().numpy())
    print(f"{name} k={k} {pre}: {res.iterations} updates (restatement {count}), margin {margin:.3f}, restatement moves {moved:.2e} under the "
          f"perturbation, history differs by {hist_diff(res.res_history, hist):.3e}, true residual {true:.3e}")
    assert status == R.OK and res.status == 0
    assert true < RTOL_SQ
    if (name, k, pre) in COUNT_CASES:
        assert margin >= 1.2, f"the stop margin of this count case shrank to {margin:.3f}"
        assert moved < 1e-11, f"the restatement's own history moves by {moved:.2e}"
    if margin >= 1.2 and moved < 1e-11:
        assert res.iterations == count
        assert hist_diff(res.res_history, hist) <= HIST_RTOL
    else:
        assert res.res_history[-1] < RTOL_SQ and res.res_history[:-1].min() >= RTOL_SQ


def test_b_in_the_deflated_span_takes_no_update(D):
    A, _ = system("33x31")
    V, _ = eigenvectors("33x31", "jacobi")
    S = attach(D, A, V[:, :3], "jacobi")
    d = S.deflation()
    b = d["AW"] @ np.array([1.0, -2.0, 0.5])
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    assert res.status == 0 and res.iterations == 0 and len(res.res_history) == 1
    assert R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ


def test_x0_cap_and_init_check_r(D):
    A, b = system("40x40")
    V, _ = eigenvectors("40x40", "jacobi")
    S = attach(D, A, V[:, :3], "jacobi")
    d = S.deflation()
    W, AW, m = d["W"], d["AW"], R.jacobi(A)
    x0 = np.random.default_rng(2).random(A.shape[0])
    res = S.solve(gpu(b), gpu(x0), rtol_sq=RTOL_SQ)
    status, count, hist, _ = R.pcg(A, b, W, AW, m, x0=x0, rtol_sq=RTOL_SQ)
    print(f"x0: {res.iterations} updates (restatement {count}, margin {R.stop_margin(hist, RTOL_SQ):.3f}), history differs by "
          f"{hist_diff(res.res_history, hist):.3e}")
    assert res.status == 0 and status == R.OK and R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ
    if R.stop_margin(hist, RTOL_SQ) >= 1.2 and stable(A, b, W, AW, m, R.pcg(A, b, W, AW, m, rtol_sq=RTOL_SQ)[2]) < 1e-11:
        assert abs(res.iterations - count) <= (0 if hist_diff(res.res_history, hist) <= HIST_RTOL else 1)
    # the cap
    res5 = S.solve(gpu(b), rtol_sq=RTOL_SQ, max_iter=5)
    _, _, hist5, x5 = R.pcg(A, b, W, AW, m, rtol_sq=RTOL_SQ, max_iter=5)
    assert res5.status == D._lib.MAX_ITER and res5.iterations == 5 and len(res5.res_history) == 6
    assert hist_diff(res5.res_history, hist5) <= HIST_RTOL
    assert np.abs(res5.x.cpu().numpy() - x5).max() <= 1e-10 * np.abs(x5).max()
    # DPCG_INIT_CHECK_R: the first entry is <r,r>/<b,b> of the corrected r
    resr = S.solve(gpu(b), rtol_sq=RTOL_SQ, flags=D._lib.INIT_CHECK_R)
    _, countr, histr, _ = R.pcg(A, b, W, AW, m, rtol_sq=RTOL_SQ, init_check_r=True)
    _, _, histz, _ = R.pcg(A, b, W, AW, m, rtol_sq=RTOL_SQ)
    assert resr.status == 0 and resr.iterations == countr and hist_diff(resr.res_history, histr) <= HIST_RTOL
    assert abs(histr[0] - histz[0]) > 1e-3 * histr[0]                                # (the two first tests differ here)


def factor_apply(S, kind):
    rp, ci, v = S.factor()
    Lf = sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))
    if kind == "ic0":
        Lc, Ltc = sp.csr_matrix(Lf), sp.csr_matrix(Lf.T)
        return lambda r: spla.spsolve_triangular(Ltc, spla.spsolve_triangular(Lc, r, lower=True), lower=False)
    return lambda r: Lf @ (Lf.T @ r)


@pytest.mark.parametrize("kind", ["ic0", "fsai"])
def test_generic_preconditioners(D, kind):
    A, b = system("40x40")
    V, _ = eigenvectors("40x40", "jacobi")
    S = attach(D, A, V[:, :3], D.IC0("solve") if kind == "ic0" else D.FSAI(level=1))
    d = S.deflation()
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    m = factor_apply(S, kind)
    status, count, hist, _ = R.pcg(A, b, d["W"], d["AW"], m, rtol_sq=RTOL_SQ)
    _, plain, _, _ = R.pcg(A, b, apply_m=m, rtol_sq=RTOL_SQ)
    margin = R.stop_margin(hist, RTOL_SQ)
    print(f"{kind}: {res.iterations} updates (restatement {count}, margin {margin:.3f}, plain {plain}), history differs by "
          f"{hist_diff(res.res_history, hist):.3e}")
    assert status == R.OK and res.status == 0 and R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ
    if margin >= 1.2 and stable(A, b, d["W"], d["AW"], m, hist) < 1e-11:
        assert res.iterations == count and hist_diff(res.res_history, hist) <= HIST_RTOL
    else:
        assert abs(res.iterations - count) <= 1


def test_amg_converges(D):
    A, b = system("40x40")
    V, _ = eigenvectors("40x40", "jacobi")
    S = attach(D, A, V[:, :3], D.SmoothedAggregation())
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    assert res.status == 0 and R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ


def test_reordered_handle(D):
    A, b = system("40x40")
    V, _ = eigenvectors("40x40", "jacobi")
    perm = np.random.default_rng(7).permutation(A.shape[0])
    B = sp.csr_matrix(A[perm][:, perm])
    B.sort_indices()
    B.indices, B.indptr = B.indices.astype(np.int32), B.indptr.astype(np.int32)
    bb = b[perm]
    S = attach(D, B, V[perm, :3], "jacobi", reorder="rcm")
    assert S.reordered and S.permutation() is not None
    d = S.deflation()
    check_orthonormal(B, d["W"], d["AW"])                                            # the caller's numbering
    res = S.solve(gpu(bb), rtol_sq=RTOL_SQ)
    plain = attach(D, A, V[:, :3], "jacobi").solve(gpu(b), rtol_sq=RTOL_SQ)
    status, count, hist, _ = R.pcg(B, bb, d["W"], d["AW"], R.jacobi(B), rtol_sq=RTOL_SQ)
    assert R.stop_margin(hist, RTOL_SQ) >= 1.2
    print(f"reordered: {res.iterations} updates (unreordered {plain.iterations}, restatement {count}), history differs by "
          f"{hist_diff(res.res_history, hist):.3e}")
    assert res.status == 0 and res.iterations == count == plain.iterations and hist_diff(res.res_history, hist) <= HIST_RTOL
    assert R.true_residual(B, bb, res.x.cpu().numpy()) < RTOL_SQ
    with pytest.raises(D._lib.DpcgError, match="deflation attached") as e:
        S2 = attach(D, A, V[:, :3], "jacobi")
        D._lib.check(D._lib.lib().dpcg_reorder(S2._h, 2, None, None))
    assert e.value.status == D._lib.ERR_STATE


def test_update_values(D):
    A, b = system("40x40")
    V, _ = eigenvectors("40x40", "jacobi")
    S = attach(D, A, V[:, :3], "jacobi")
    before = S.deflation()
    drift = 1.0 + 0.2 * np.random.default_rng(4).random(A.shape[0])                  # A2 = D A D: same pattern, drifted values
    A2 = sp.csr_matrix(sp.diags(drift) @ A @ sp.diags(drift))
    A2.sort_indices()
    assert np.array_equal(A2.indices, A.indices)
    S.update_values(A2.data)
    S.set_preconditioner(D.Jacobi())
    d = S.deflation()
    assert d is not None and d["k"] == 3
    check_orthonormal(A2, d["W"], d["AW"])
    # the span is kept: the new W lies in the span of the old one
    coef, *_ = np.linalg.lstsq(before["W"], d["W"], rcond=None)
    assert np.abs(before["W"] @ coef - d["W"]).max() <= 1e-10 * np.abs(d["W"]).max()
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    status, count, hist, _ = R.pcg(A2, b, d["W"], d["AW"], R.jacobi(A2), rtol_sq=RTOL_SQ)
    margin = R.stop_margin(hist, RTOL_SQ)
    print(f"drifted values: {res.iterations} updates (restatement {count}, margin {margin:.3f}), history differs by "
          f"{hist_diff(res.res_history, hist):.3e}")
    assert status == R.OK and res.status == 0 and R.true_residual(A2, b, res.x.cpu().numpy()) < RTOL_SQ
    if margin >= 1.2:
        assert res.iterations == count and hist_diff(res.res_history, hist) <= HIST_RTOL
    else:
        assert abs(res.iterations - count) <= 1
    # values under which a column vanishes in the A inner product: the deflation is dropped and the call says so
    with pytest.raises(D._lib.DpcgError, match="dropped") as e:
        S.update_values(np.zeros_like(A.data))
    assert e.value.status == D._lib.ERR_INVALID and S.deflation() is None


def test_solve_refusals(D):
    A, b = system("5x7")
    V, _ = eigenvectors("5x7", "jacobi")
    bt = gpu(b)
    S = attach(D, A, V[:, :3], "jacobi")
    for kw, what in ((dict(recurrence="single_reduction"), "SINGLE_REDUCTION"), (dict(flags=D._lib.SPMV_F32), "SPMV_F32"),
                     (dict(flags=D._lib.TEAM), "DPCG_TEAM"), (dict(x_true=bt), "x_true")):
        with pytest.raises(D._lib.DpcgError, match=what) as e:
            S.solve(bt, **kw)
        assert e.value.status == D._lib.ERR_INVALID and "deflation" in str(e.value)
    from deeppreconditioning_amd.batch import solve_batch
    S2 = D.CsrSystem.from_any(A, reorder=None)
    with pytest.raises(D._lib.DpcgError, match="deflation") as e:
        solve_batch([S2, S], [bt, bt])
    assert e.value.status == D._lib.ERR_INVALID

    class Op:
        def __matmul__(self, r):
            return r

    S.set_preconditioner(D.OperatorPreconditioner(Op()))
    with pytest.raises(D._lib.DpcgError, match="callback") as e:
        S.solve(bt)
    assert e.value.status == D._lib.ERR_INVALID
    S.set_preconditioner(D.Jacobi())
    # a null space and a deflation: refused at whichever attach comes second
    with pytest.raises(D._lib.DpcgError, match="deflation attached") as e:
        S.set_nullspace("constant", check_tol=0.0)
    assert e.value.status == D._lib.ERR_INVALID and S.nullspace() is None
    S3 = D.CsrSystem.from_any(A, reorder=None)
    S3.set_nullspace("constant", check_tol=0.0)
    with pytest.raises(D._lib.DpcgError, match="null space attached") as e:
        S3.set_deflation(V[:, :3])
    assert e.value.status == D._lib.ERR_INVALID and S3.deflation() is None
    assert S.solve(bt, rtol_sq=RTOL_SQ).status == 0                                  # the handle is untouched by the refusals


def test_attach_refusals_and_clearing(D):
    A, b = system("33x31")
    V, _ = eigenvectors("33x31", "jacobi")
    bt = gpu(b)
    S = attach(D, A, None, "jacobi")
    plain = S.solve(bt, rtol_sq=RTOL_SQ)
    S.set_deflation(V[:, :3])
    kept = S.deflation()
    with_w = S.solve(bt, rtol_sq=RTOL_SQ)
    assert with_w.iterations < plain.iterations
    dup = V[:, :3].copy()
    dup[:, 2] = dup[:, 0]
    nan = V[:, :3].copy()
    nan[17, 1] = np.nan
    for bad, what in ((dup, "column 2"), (nan, "non-finite"), (np.random.default_rng(0).random((A.shape[0], 9)), "k must lie")):
        with pytest.raises(D._lib.DpcgError, match=what) as e:
            S.set_deflation(bad)
        assert e.value.status == D._lib.ERR_INVALID
        now = S.deflation()                                                          # the handle keeps what it had
        assert now["k"] == 3 and np.array_equal(now["W"], kept["W"]) and np.array_equal(now["AW"], kept["AW"])
        again = S.solve(bt, rtol_sq=RTOL_SQ)
        assert again.iterations == with_w.iterations and np.array_equal(again.res_history, with_w.res_history)
    with pytest.raises(D._lib.DpcgError, match="k must lie"):
        D._lib.check(D._lib.lib().dpcg_set_deflation(S._h, -1, None, D._lib.HOST, None))
    S.set_deflation(None)
    assert S.deflation() is None
    back = S.solve(bt, rtol_sq=RTOL_SQ)
    assert back.iterations == plain.iterations and np.array_equal(back.res_history, plain.res_history)
    assert np.array_equal(back.x.cpu().numpy(), plain.x.cpu().numpy())


def test_subdomain_indicators_and_cg_keyword(D):
    from deeppreconditioning_amd.cg import conjugate_gradient, preconditioned_conjugate_gradient
    A, b = system("40x40")
    Wi = subdomain_indicators((40, 40), (2, 4))
    plain = preconditioned_conjugate_gradient(A, torch.from_numpy(b), D.Jacobi(), details=True)
    res = preconditioned_conjugate_gradient(A, torch.from_numpy(b), D.Jacobi(), deflation=Wi, details=True)
    assert res.status == 0 and res.iterations < plain.iterations and R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ
    errors, x_hat = conjugate_gradient(A, torch.from_numpy(b), deflation=Wi)
    assert float(errors[-1][1]) < RTOL_SQ and len(errors) - 1 < plain.iterations
    assert R.true_residual(A, b, x_hat.cpu().numpy()) < RTOL_SQ


def numpy_ritz(A, dinv, seed, steps, k):
    """The restatement of the harvest: `steps` Lanczos steps in the M inner product with full CGS2, numpy's own sums; the k lowest
    Ritz values, their bounds beta_{m+1} |s_m| and the Ritz vectors y_i = Z s_i."""
    n = A.shape[0]
    v = LZ._hash(seed, np.arange(n))
    u = dinv * v
    nrm = np.sqrt(v @ u)
    Rb, Zb = [v / nrm], [u / nrm]
    alpha, beta = [], [0.0]
    for j in range(steps):
        w = A @ Zb[j]
        alpha.append(Zb[j] @ w)
        w = w - alpha[j] * Rb[j] - (beta[j] * Rb[j - 1] if j > 0 else 0.0)
        Zm, Rm = np.array(Zb).T, np.array(Rb).T
        for _ in range(2):
            w = w - Rm @ (Zm.T @ w)
        u = dinv * w
        beta.append(np.sqrt(max(w @ u, 0.0)))
        if beta[-1] == 0.0:
            break
        Rb.append(w / beta[-1])
        Zb.append(u / beta[-1])
    m = len(alpha)
    T = np.diag(alpha) + np.diag(beta[1:m], 1) + np.diag(beta[1:m], -1)
    theta, Sv = np.linalg.eigh(T)
    Y = np.array(Zb[:m]).T @ Sv[:, :k]
    return theta[:k], beta[m] * np.abs(Sv[m - 1, :k]), Y


def test_harvest(D):
    A, b = system("w32x32")
    n = A.shape[0]
    dinv = 1.0 / A.diagonal()
    V, lam = eigenvectors("w32x32", "jacobi")
    assert np.diff(lam[:5]).min() > 1e-5 * lam[-1], "the five lowest eigenvalues must be distinct: use another seed"
    S = attach(D, A, None, "jacobi")
    S.set_deflation("ritz", k=4, max_steps=n, rtol=1e-6, seed=0)
    d = S.deflation()
    theta, err, steps = d["theta"], d["err"], d["steps"]
    print(f"harvest: {steps} steps, theta {theta}, err {err}, exact {lam[:4]}")
    assert d["k"] == 4 and d["converged"] and np.all(np.diff(theta) > 0)
    assert np.all(np.abs(theta - lam[:4]) <= err + 1e-10 * lam[-1])
    # the raw Ritz vectors, as dpcg_spectrum_vectors leaves them
    import ctypes as C
    Wd = torch.empty(n * 4, dtype=torch.float64, device="cuda")
    th2, er2, st2 = np.zeros(4), np.zeros(4), C.c_int(0)
    status = D._lib.check(D._lib.lib().dpcg_spectrum_vectors(S._h, 4, n, 1e-6, 0, None, C.byref(st2), th2.ctypes.data, er2.ctypes.data,
                                                            Wd.data_ptr()))
    torch.cuda.synchronize()
    assert status == D._lib.OK and st2.value == steps and np.array_equal(th2, theta) and np.array_equal(er2, err)
    Y = Wd.cpu().numpy().reshape(4, n).T
    rt, re, Yr = numpy_ritz(A, dinv, 0, steps, 4)
    res_dev = np.linalg.norm(dinv[:, None] * (A @ Y) - Y * theta[None, :], axis=0)
    res_ref = np.linalg.norm(dinv[:, None] * (A @ Yr) - Yr * rt[None, :], axis=0)
    scale = np.sqrt(dinv.max())
    slack = 4.0 * np.maximum(res_ref - re * scale, 0.0)                              # what rounding adds to the restatement's own check
    print(f"Ritz residuals {res_dev}, bounds {err * scale}, restatement {res_ref} against {re * scale}, slack {slack}")
    assert np.all(res_dev <= err * scale + slack)
    # the harvested space deflates as the exact eigenvectors do
    res = S.solve(gpu(b), rtol_sq=RTOL_SQ)
    We, AWe = R.a_orthonormalise(A, V[:, :4])
    _, exact, _, _ = R.pcg(A, b, We, AWe, R.jacobi(A), rtol_sq=RTOL_SQ)
    print(f"ritz deflation: {res.iterations} updates, restatement with exact eigenvectors {exact}")
    assert res.status == 0 and abs(res.iterations - exact) <= 1 and R.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ
    # max_steps too small: DPCG_MAX_ITER, and the vectors are still returned
    S.set_deflation("ritz", k=4, max_steps=8, rtol=1e-12)
    d = S.deflation()
    assert d["k"] == 4 and d["steps"] == 8 and not d["converged"]
