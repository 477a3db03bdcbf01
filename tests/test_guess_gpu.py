"""The projected initial guess on the device (dpcg_guess_*, `ProjectedGuess`, `CsrSystem.solve(guess=)`) against its numpy
restatement (tests/guess_restatement.py) and through the solver.

Yardstick of the device-equals-restatement tests: the restatement is run twice, with sequential and with pairwise sums -- two
legitimate orders of the same algorithm; the device (per-wave partials, then one fixed order) is a third.  The bar for a case is
8 x the largest distance between those two runs over the steps of the sequence, for x0 relative to ||x0|| and for the basis
relative to its Frobenius norm; info() has to agree exactly.  The distance of a single step is one draw of a rounding error and
no yardstick by itself: over these cases the two orders round a step's result to the very same bits in 38 of 765 comparisons
with n > 1, and a third host order (sums over blocks of 128 rows, then first to last) lies up to 1.5 x beyond 8 x its own step's
distance -- hence the largest over the sequence.  Shapes put rows on both sides of a wave (63, 65), of a workgroup
(256, 729), of the 1024-row padding (1023, 1025, 4097) and n = 1; depths 1 and 2 restart inside six solves, 7 and 8 bracket the
register width of the triangular multiply, 32 is the limit (test_deep_basis fills 20 of its columns).
"""

import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import guess_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
INFO_KEYS = ("depth", "size", "restarts", "appended", "skipped", "dropped", "reorthonormalisations", "values_epoch")


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def grid_poisson(mx, my):
    tx = sp.diags([-np.ones(mx - 1), 2.0 * np.ones(mx), -np.ones(mx - 1)], [-1, 0, 1])
    ty = sp.diags([-np.ones(my - 1), 2.0 * np.ones(my), -np.ones(my - 1)], [-1, 0, 1])
    return _csr(sp.kron(sp.identity(my), tx) + sp.kron(ty, sp.identity(mx)))


def tridiagonal(n):
    d = 2.5 + 0.5 * np.sin(np.arange(n))
    if n == 1:
        return _csr(sp.csr_matrix(np.array([[d[0]]])))
    return _csr(sp.diags([-np.ones(n - 1), d, -np.ones(n - 1)], [-1, 0, 1]))


SHAPES = {"poisson2d_16x16": lambda: grid_poisson(16, 16), "poisson2d_33x31": lambda: grid_poisson(33, 31),
          "poisson3d_9": lambda: _csr(O.poisson3d(9)), "tri_1": lambda: tridiagonal(1), "tri_63": lambda: tridiagonal(63),
          "tri_65": lambda: tridiagonal(65), "tri_1023": lambda: tridiagonal(1023), "tri_1025": lambda: tridiagonal(1025),
          "tri_4097": lambda: tridiagonal(4097)}
DEPTHS = (1, 2, 7, 8, 32)


def rescaled(A, phase):
    """Another SPD matrix on A's pattern: D^1/2 A D^1/2 + 0.1 I with a smooth D."""
    n = A.shape[0]
    s = sp.diags(np.sqrt(1.0 + 0.4 * np.sin(phase + np.arange(n) * (6.0 / max(n, 6)))))
    B = _csr(s @ A @ s + 0.1 * sp.identity(n))
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)
    return B


_SEQUENCES = {}


def sequence(shape, depth, solves, change_at):
    """The inputs of a case and both restatement runs, computed once: per step (A or None, b, x, x0_seq, info_seq, basis_seq) and
    the two distances between the sequential and the pairwise run."""
    key = (shape, depth, solves, change_at)
    if key in _SEQUENCES:
        return _SEQUENCES[key]
    A = SHAPES[shape]()
    n = A.shape[0]
    rng = np.random.default_rng(1000 * depth + n)
    runs = {sums: R.Guess(A, depth=depth, tol_dep=1e-7, sums=sums) for sums in ("sequential", "pairwise")}
    steps, dist_x0, dist_basis = [], 0.0, 0.0
    cur = A
    for k in range(solves):
        new = None
        if k in change_at:
            cur = new = rescaled(A, 0.7 * k)
            for g in runs.values():
                g.set_matrix(cur)
        b = rng.standard_normal(n)
        x = spla.spsolve(sp.csc_matrix(cur), b) if n > 1 else b / cur.toarray()[0]
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        x0 = {s: g.project(b) for s, g in runs.items()}
        info_p = runs["sequential"].info()
        assert runs["pairwise"].info() == info_p
        for g in runs.values():
            g.update(x)
        info_u = runs["sequential"].info()
        assert runs["pairwise"].info() == info_u, "the two orders disagree about a decision: the case sits on a threshold"
        nx = np.linalg.norm(x0["sequential"])
        if nx > 0:
            dist_x0 = max(dist_x0, np.linalg.norm(x0["sequential"] - x0["pairwise"]) / nx)
        bs, bp = runs["sequential"].basis(), runs["pairwise"].basis()
        for m_s, m_p in zip(bs, bp):
            if m_s.size:
                dist_basis = max(dist_basis, np.linalg.norm(m_s - m_p) / np.linalg.norm(m_s))
        steps.append((new, b, x, x0["sequential"], info_p, info_u, bs))
    _SEQUENCES[key] = (A, steps, dist_x0, dist_basis)
    return _SEQUENCES[key]


def device_info(g):
    i = g.info()
    return {k: i[k] for k in INFO_KEYS}


def run_on_device(D, A, steps, depth, reorder="none"):
    """The same sequence on the device: per step (x0, info after project, info after update, basis)."""
    S = D.CsrSystem.from_any(A, reorder=reorder)
    g = D.ProjectedGuess(S, depth=depth, tol_dep=1e-7)
    out = []
    for new, b, x, *_ in steps:
        if new is not None:
            S.update_values(new.data)
        x0 = g.project(b).cpu().numpy()
        ip = device_info(g)
        g.update(x)
        out.append((x0, ip, device_info(g), g.basis()))
    g.close()
    S.close()
    return out


def compare(dev, steps, dist_x0, dist_basis, label):
    worst_x0 = worst_basis = 0.0
    for (x0, ip, iu, (X, W)), (_, _, _, x0_ref, info_p, info_u, (Xr, Wr)) in zip(dev, steps):
        assert ip == {k: info_p[k] for k in INFO_KEYS} and iu == {k: info_u[k] for k in INFO_KEYS}
        nx = np.linalg.norm(x0_ref)
        if nx > 0:
            worst_x0 = max(worst_x0, np.linalg.norm(x0 - x0_ref) / nx)
        else:
            assert not x0.any()
        for m, mr in ((X, Xr), (W, Wr)):
            assert m.shape == mr.shape
            if mr.size:
                worst_basis = max(worst_basis, np.linalg.norm(m - mr) / np.linalg.norm(mr))
    print(f"{label}: x0 device-restatement {worst_x0:.3e} bar {8 * dist_x0:.3e} | basis {worst_basis:.3e} bar {8 * dist_basis:.3e}")
    assert worst_x0 <= 8 * dist_x0
    assert worst_basis <= 8 * dist_basis


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_equals_restatement(D, shape, depth):
    """Six solves, new matrix values before the fifth.  Measured on an MI355X over the 45 cases (relative): x0 differs from the
    sequential restatement by at most 2.1e-14 where the bars (8 x the distance between the sequential and the pairwise run) lie
    between 3.1e-15 and 2.7e-13 -- at most 0.35 of its bar in any case; the basis by at most 1.7e-15 against bars of 1.6e-15 ..
    1.3e-14, at most 0.20 of its bar.  n = 1: both distances are 0 and the device gives the restatement's bits."""
    A, steps, dist_x0, dist_basis = sequence(shape, depth, 6, (4,))
    compare(run_on_device(D, A, steps, depth), steps, dist_x0, dist_basis, f"{shape} depth {depth}")


def test_deep_basis(D):
    """Depth 32 with twenty columns in use and new values before solves 10 and 18: the 16- and 32-wide triangular multiplies and
    dot products over more than eight columns.  Measured on an MI355X: x0 2.0e-15 against a bar of 1.2e-14, the basis 1.3e-15
    against 9.9e-15."""
    A, steps, dist_x0, dist_basis = sequence("poisson2d_33x31", 32, 20, (9, 17))
    dev = run_on_device(D, A, steps, 32)
    assert dev[-1][2]["size"] == 20
    compare(dev, steps, dist_x0, dist_basis, "deep basis")


def test_numbering(D):
    """A handle that iterates in reverse Cuthill-McKee order gives the x0 and the basis of one that does not, within the bar of the
    case, and the basis is in the caller's numbering (it is compared row by row with the restatement's)."""
    A, steps, dist_x0, dist_basis = sequence("poisson2d_33x31", 8, 6, (4,))
    S = D.CsrSystem.from_any(A, reorder="rcm")
    assert S.reordered
    S.close()
    plain = run_on_device(D, A, steps, 8, reorder="none")
    rcm = run_on_device(D, A, steps, 8, reorder="rcm")
    compare(rcm, steps, dist_x0, dist_basis, "rcm")
    for (a, _, ia, (Xa, Wa)), (b, _, ib, (Xb, Wb)) in zip(plain, rcm):
        assert ia == ib
        if np.linalg.norm(a) > 0:
            assert np.linalg.norm(a - b) <= 8 * dist_x0 * np.linalg.norm(a)
        if Xa.size:
            assert np.linalg.norm(Xa - Xb) <= 8 * dist_basis * np.linalg.norm(Xa)
            assert np.linalg.norm(Wa - Wb) <= 8 * dist_basis * np.linalg.norm(Wa)


def test_determinism(D):
    A, steps, _, _ = sequence("tri_4097", 7, 6, (4,))
    one = run_on_device(D, A, steps, 7)
    two = run_on_device(D, A, steps, 7)
    for (a, _, ia, (Xa, Wa)), (b, _, ib, (Xb, Wb)) in zip(one, two):
        assert ia == ib
        assert a.tobytes() == b.tobytes() and Xa.tobytes() == Xb.tobytes() and Wa.tobytes() == Wb.tobytes()


def test_unaligned_vectors(D):
    """b, x0 and x at addresses that are 8 but not 16 bytes aligned (views that start at element 1) take the row-by-row path of the
    kernels for the whole vector: same bits as the aligned calls.  n = 1025 also has a partial last group on the aligned path."""
    from deeppreconditioning_amd.operators import _dev_ptr, _stream
    A, steps, _, _ = sequence("tri_1025", 7, 6, (4,))
    n = A.shape[0]
    systems = [D.CsrSystem.from_any(A, reorder="none") for _ in range(2)]
    aligned, shifted = (D.ProjectedGuess(S, depth=7) for S in systems)

    def view(values=None):
        t = torch.zeros(n + 1, dtype=torch.float64, device="cuda")[1:]
        assert t.data_ptr() % 16 == 8 and t.is_contiguous()
        if values is not None:
            t.copy_(torch.from_numpy(values))
        return t

    for new, b, x, *_ in steps:
        if new is not None:
            for S in systems:
                S.update_values(new.data)
        x0_a = aligned.project(b)
        aligned.update(x)
        bv, x0_v, xv = view(b), view(), view(x)
        D._lib.check(D._lib.lib().dpcg_guess_project(shifted._g, _dev_ptr(bv), _dev_ptr(x0_v), _stream()))
        shifted.update(xv)
        assert torch.equal(x0_a, x0_v)
        (Xa, Wa), (Xs, Ws) = aligned.basis(), shifted.basis()
        assert aligned.info() == shifted.info() and Xa.tobytes() == Xs.tobytes() and Wa.tobytes() == Ws.tobytes()
    assert aligned.info()["size"] == 6
    for S in systems:
        S.close()


def test_breakdown_leaves_the_basis_alone(D):
    """solve(guess=) hands nothing to the basis when the solve broke down (b = 0: <b, b> = 0 makes the first test 0 / 0)."""
    A = grid_poisson(16, 16)
    S = D.CsrSystem.from_any(A)
    g = D.ProjectedGuess(S, depth=4)
    S.solve(np.ones(256), guess=g)
    info, (X, W) = g.info(), g.basis()
    r = S.solve(np.zeros(256), guess=g)
    assert r.status == D._lib.BREAKDOWN
    assert g.info() == info and g.basis()[0].tobytes() == X.tobytes() and g.basis()[1].tobytes() == W.tobytes()
    S.close()


def test_exact_recovery(D):
    """b3 = 2 b1 - 3 b2 after b1 and b2 were solved to rtol_sq = 1e-24: the projection is the solution, and the solve at
    rtol_sq = 1e-16 reports 0 iterations under DPCG_INIT_CHECK_R (the pair of tolerances the issue names; fp64 reaches both)."""
    A = grid_poisson(16, 16)
    rng = np.random.default_rng(5)
    b1, b2 = rng.standard_normal(256), rng.standard_normal(256)
    S = D.CsrSystem.from_any(A)
    g = D.ProjectedGuess(S, depth=8)
    for b in (b1, b2):
        r = S.solve(b, rtol_sq=1e-24, flags=D._lib.INIT_CHECK_R, guess=g)
        assert r.status == D._lib.OK and r.final_res < 1e-24
    assert g.info()["size"] == 2
    b3 = 2.0 * b1 - 3.0 * b2
    with_guess = S.solve(b3, rtol_sq=1e-16, flags=D._lib.INIT_CHECK_R, guess=g)
    without = S.solve(b3, rtol_sq=1e-16, flags=D._lib.INIT_CHECK_R)
    print("exact recovery: iterations", with_guess.iterations, "against", without.iterations, "first residual", with_guess.final_res)
    assert with_guess.status == D._lib.OK and with_guess.iterations == 0
    assert without.iterations > 0
    x = with_guess.x.cpu().numpy()
    assert np.linalg.norm(A @ x - b3) <= 1e-8 * np.linalg.norm(b3)
    assert g.info()["size"] == 2 and g.info()["skipped"] == 1           # the third solution lies in the span


def changing_step(m, t, A0):
    xs = (np.arange(m) + 0.5) / m
    xg, yg = np.meshgrid(xs, xs, indexing="xy")
    coeff = (1.0 + 0.5 * np.sin(2 * np.pi * (xg - 0.02 * t)) * np.cos(2 * np.pi * yg)).ravel()
    s = sp.diags(np.sqrt(coeff))
    A = _csr(s @ A0 @ s + 0.05 * sp.identity(m * m))
    b = (np.sin(np.pi * xg) * np.sin(np.pi * yg) * (1 + 0.1 * t) + 0.3 * np.sin(2 * np.pi * (xg + 0.03 * t)) * yg).ravel()
    return A, b


def test_changing_matrix(D):
    """A_t = D_t^1/2 A D_t^1/2 + 0.05 I on a 40 x 40 grid, the coefficient field D_t = 1 + 0.5 sin 2 pi (x - 0.02 t) cos 2 pi y
    drifting, the right-hand side varying smoothly; 8 steps through update_values, M = I, rtol_sq = 1e-16, depth 8.
    On the CPU (the restatement with the oracle's PCG, first test on r) the updates of steps 3 .. 8 sum to 387 with the guess
    against 603 without, 1.56 x fewer; per step 102 95 86 75 65 57 53 51 against 102 103 102 102 101 100 99 99.
    Orthonormality bound: n eps kappa(A_t) as in tests/test_guess_host.py with kappa <= (1.5 x 8 + 0.05) / (0.05 + 0.5 x 0.0117) = 216
    (Gershgorin above, the smallest eigenvalue of the 40 x 40 Laplacian, 4 (1 - cos(pi / 41)), scaled by min D_t below)."""
    m = 40
    A0 = grid_poisson(m, m)
    S = D.CsrSystem.from_any(changing_step(m, 1, A0)[0])
    plain = D.CsrSystem.from_any(changing_step(m, 1, A0)[0])
    g = D.ProjectedGuess(S, depth=8)
    rtol_sq = 1e-16
    with_guess, without = [], []
    for t in range(1, 9):
        A, b = changing_step(m, t, A0)
        S.update_values(A.data)
        plain.update_values(A.data)
        r = S.solve(b, rtol_sq=rtol_sq, max_iter=4000, flags=D._lib.INIT_CHECK_R, guess=g)
        q = plain.solve(b, rtol_sq=rtol_sq, max_iter=4000, flags=D._lib.INIT_CHECK_R)
        assert r.status == D._lib.OK and q.status == D._lib.OK
        x, y = r.x.cpu().numpy(), q.x.cpu().numpy()
        # both residuals are below sqrt(rtol_sq) ||b||; the recurrences' drift from the true residuals is of the order eps ||A|| ||x||
        assert np.linalg.norm(A @ (x - y)) <= 2 * math.sqrt(rtol_sq) * np.linalg.norm(b) + 64 * EPS * 12.05 * np.linalg.norm(x)
        info = g.info()
        assert info["reorthonormalisations"] == t and info["values_epoch"] == t and info["dropped"] == 0
        assert info["size"] == min(t, 8)
        X, W = g.basis()
        assert np.max(np.abs(X.T @ (A @ X) - np.eye(X.shape[1]))) <= m * m * EPS * 216
        with_guess.append(r.iterations)
        without.append(q.iterations)
    print("changing matrix: updates with the guess", with_guess, "without", without)
    assert sum(with_guess[2:]) < sum(without[2:])
    S.close()
    plain.close()


def test_restart_and_dependence(D):
    A = grid_poisson(16, 16)
    rng = np.random.default_rng(11)
    S = D.CsrSystem.from_any(A)
    g = D.ProjectedGuess(S, depth=2)
    sizes = []
    for _ in range(5):
        S.solve(rng.standard_normal(256), rtol_sq=1e-20, guess=g)
        sizes.append(g.info()["size"])
    assert sizes == [1, 2, 1, 2, 1] and g.info()["restarts"] == 2
    g.reset()
    assert g.info()["size"] == 0 and g.info()["restarts"] == 0
    b = rng.standard_normal(256)
    first = S.solve(b, rtol_sq=1e-20, guess=g)
    X1, W1 = g.basis()
    second = S.solve(b, rtol_sq=1e-20, guess=g)
    info = g.info()
    assert info["size"] == 1 and info["skipped"] == 1 and info["appended"] == 1
    X2, W2 = g.basis()
    assert X1.tobytes() == X2.tobytes() and W1.tobytes() == W2.tobytes()
    assert np.all(np.isfinite(X2)) and np.all(np.isfinite(W2)) and torch.isfinite(second.x).all()
    assert second.iterations < first.iterations


@pytest.mark.parametrize("form", ["chip", "small"])
def test_one_launch_forms(D, form):
    """A 41^3 system is solved by the whole chip in one launch, a 64 x 64 one by one workgroup: both take the projected x0, and a
    solve capped at three updates still hands its iterate to the basis."""
    A = _csr(O.poisson3d(41)) if form == "chip" else grid_poisson(64, 64)
    n = A.shape[0]
    assert n == (68921 if form == "chip" else 4096)
    S = D.CsrSystem.from_any(A)
    if form == "chip":
        assert S.chip_info()["chip_by_default"]
    else:
        assert S.reduction_geometry()["small_threads"] > 0
    g = D.ProjectedGuess(S, depth=4)
    xs = (np.arange(n) + 0.5) / n
    iters = []
    for t in range(3):
        b = np.sin(2 * np.pi * (xs + 0.01 * t)) + 0.5 * np.cos(6 * np.pi * xs) * (1 + 0.05 * t)
        r = S.solve(b, rtol_sq=1e-16, max_iter=2000, guess=g)
        assert r.status == D._lib.OK
        assert np.linalg.norm(A @ r.x.cpu().numpy() - b) <= 2e-8 * np.linalg.norm(b)
        iters.append(r.iterations)
    print(form, "updates per solve", iters)
    assert g.info()["size"] == 3 and iters[2] < iters[0]
    capped = S.solve(np.cos(4 * np.pi * xs), rtol_sq=1e-16, max_iter=3, guess=g)
    assert capped.status == D._lib.MAX_ITER and capped.iterations == 3
    assert g.info()["size"] == 4
    X, W = g.basis()
    m = 41 if form == "chip" else 64
    kappa = (2 * (m + 1) / math.pi) ** 2                          # cot^2(pi / (2 (m + 1))), the grid Laplacian's condition number
    assert np.max(np.abs(X.T @ (A @ X) - np.eye(4))) <= n * EPS * kappa         # (the bound of tests/test_guess_host.py)
    S.close()


def test_refusals(D):
    A = grid_poisson(16, 16)
    S = D.CsrSystem.from_any(A)
    for depth in (0, 33):
        with pytest.raises(D._lib.DpcgError) as exc:
            D.ProjectedGuess(S, depth=depth)
        assert exc.value.status == D._lib.ERR_INVALID
    for tol in (0.0, -1e-7):
        with pytest.raises(D._lib.DpcgError) as exc:
            D.ProjectedGuess(S, tol_dep=tol)
        assert exc.value.status == D._lib.ERR_INVALID
    g = D.ProjectedGuess(S, depth=4)
    b = np.ones(256)
    S.solve(b, guess=g)
    before = g.basis()
    info = g.info()
    with pytest.raises(ValueError):
        g.project(np.ones(255))
    with pytest.raises(ValueError):
        g.update(np.ones(257))
    with pytest.raises(ValueError):
        S.solve(b, x0=np.zeros(256), guess=g)
    other = D.CsrSystem.from_any(A)
    with pytest.raises(ValueError):
        other.solve(b, guess=g)
    bad = b.copy()
    bad[100] = np.nan
    for call in (g.project, g.update):
        with pytest.raises(D._lib.DpcgError) as exc:
            call(bad)
        assert exc.value.status == D._lib.ERR_INVALID
    bad[100] = np.inf
    with pytest.raises(D._lib.DpcgError):
        g.project(bad)
    after = g.basis()
    assert g.info() == info and before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    S.close()
    for call in (lambda: g.project(b), lambda: g.update(b), g.info, g.basis, g.reset):
        with pytest.raises(D._lib.DpcgError) as exc:
            call()
        assert exc.value.status == D._lib.ERR_STATE
    g.close()
    other.close()
