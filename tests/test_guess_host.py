"""The projected initial guess as restated in tests/guess_restatement.py (CPU): the projection is the A-norm-best approximation
in the span of the raw earlier solutions, the invariants X~^T A X~ = I and W = A X~ hold after every kind of step, and the two
drop rules fire.

Bounds.  eps = 2^-53.  kappa = cond(A), computed here from the dense matrix.
  * best approximation: the closed form X (X^T A X)^-1 X^T b solves l x l normal equations, which loses cond(X^T A X) digits; the
    Gram-Schmidt basis does not.  The distance in the A norm, relative to ||x0||_A, is bounded by 100 eps cond(X^T A X): the
    conditioning as this test computes it, times a constant for the l <= 5 dimensions and the norm equivalences.
  * invariants: an A inner product of two A-normal vectors is a sum of n products of size <= ||A|| |x_i| |x_j| <= kappa, each
    rounded to eps: |<x~_i, A x~_j> - delta_ij| <= n eps kappa; the same bound, relative to ||A x~_j||, serves W = A X~ (the
    update forms W's column as A d - W g instead of A (d - X~ g); the cancellation in d is at most sqrt(kappa) for the
    independent solutions used here).
"""

import numpy as np
import pytest
import scipy.sparse as sp

import guess_restatement as R

EPS = 2.0 ** -53


def random_spd(n, seed):
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=np.random.RandomState(seed), format="csr")
    A = B + B.T
    A = A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(0.05, 1.0, n))
    return sp.csr_matrix(A)


def kappa(A):
    ev = np.linalg.eigvalsh(A.toarray())
    return ev[-1] / ev[0]


def check_invariants(G, A):
    X, W = G.basis()
    n, l = X.shape
    bound = n * EPS * kappa(A)
    if l == 0:
        return 0.0
    AX = A @ X
    orth = np.max(np.abs(X.T @ AX - np.eye(l)))
    cons = max(np.linalg.norm(W[:, j] - AX[:, j]) / np.linalg.norm(AX[:, j]) for j in range(l))
    assert orth <= bound, (orth, bound)
    assert cons <= bound, (cons, bound)
    return max(orth, cons)


@pytest.mark.parametrize("sums", ["sequential", "pairwise"])
@pytest.mark.parametrize("n,seed", [(50, 0), (123, 1), (300, 2)])
def test_projection_is_the_best_approximation_in_the_span(n, seed, sums):
    A = random_spd(n, seed)
    rng = np.random.default_rng(100 + seed)
    G = R.Guess(A, depth=8, tol_dep=1e-7, sums=sums)
    raw = []
    for k in range(5):
        b = rng.standard_normal(n)
        x0 = G.project(b)
        if raw:
            X = np.column_stack(raw)
            gram = X.T @ (A @ X)
            ref = X @ np.linalg.solve(gram, X.T @ b)
            e = x0 - ref
            dist = np.sqrt(e @ (A @ e)) / np.sqrt(ref @ (A @ ref))
            bound = 100 * EPS * np.linalg.cond(gram)
            print(f"n={n} l={len(raw)} dist={dist:.3e} bound={bound:.3e}")
            assert dist <= bound
        else:
            assert not x0.any()
        x = np.linalg.solve(A.toarray(), b)
        G.update(x)
        raw.append(x)
        assert G.info()["size"] == k + 1


def test_xax_identity():
    """<x, A x> = |c + g|^2 + s, the form the update uses for the dependence test."""
    A = random_spd(80, 7)
    rng = np.random.default_rng(7)
    G = R.Guess(A, depth=4)
    for _ in range(3):
        b = rng.standard_normal(80)
        G.project(b)
        x = np.linalg.solve(A.toarray(), b)
        X, W = G.basis()
        d = x - G.x0
        coeff = G.c + X.T @ (A @ d)
        d_perp = d - X @ (X.T @ (A @ d))
        assert np.isclose(coeff @ coeff + d_perp @ (A @ d_perp), R.xax_direct(A, x), rtol=1e-10)
        G.update(x)


@pytest.mark.parametrize("sums", ["sequential", "pairwise"])
def test_invariants_after_update_restart_and_skip(sums):
    n = 150
    A = random_spd(n, 3)
    Ad = A.toarray()
    rng = np.random.default_rng(3)
    G = R.Guess(A, depth=3, tol_dep=1e-7, sums=sums)
    sizes = []
    for k in range(7):
        b = rng.standard_normal(n)
        G.project(b)
        G.update(np.linalg.solve(Ad, b))
        check_invariants(G, A)
        sizes.append(G.info()["size"])
    assert sizes == [1, 2, 3, 1, 2, 3, 1]
    assert G.info()["restarts"] == 2 and G.info()["appended"] == 5
    # an exactly repeated solution is dependent: skipped, nothing changes
    b = rng.standard_normal(n)
    x = np.linalg.solve(Ad, b)
    for expect_skipped in (0, 1):
        G.project(b)
        before = G.basis()
        G.update(x)
        assert G.info()["skipped"] == expect_skipped
    assert G.info()["size"] == 2
    assert np.array_equal(before[0], G.basis()[0]) and np.array_equal(before[1], G.basis()[1])
    check_invariants(G, A)
    # another solution inside the span, handed over without a project of its own (the kept x0 is still valid)
    X, _ = G.basis()
    G.update(X @ np.array([0.3, -2.0]))
    assert G.info()["skipped"] == 2 and G.info()["size"] == 2


@pytest.mark.parametrize("sums", ["sequential", "pairwise"])
def test_invariants_after_a_changed_matrix(sums):
    n = 200
    A = random_spd(n, 4)
    rng = np.random.default_rng(4)
    G = R.Guess(A, depth=6, sums=sums)
    for k in range(4):
        b = rng.standard_normal(n)
        G.project(b)
        G.update(np.linalg.solve(A.toarray(), b))
    scale = sp.diags(np.sqrt(1.0 + 0.5 * np.sin(np.arange(n) / 9.0)))
    A2 = sp.csr_matrix(scale @ A @ scale + 0.1 * sp.identity(n))
    G.set_matrix(A2)
    b = rng.standard_normal(n)
    x0 = G.project(b)
    info = G.info()
    assert info["reorthonormalisations"] == 1 and info["dropped"] == 0 and info["size"] == 4 and info["values_epoch"] == 1
    check_invariants(G, A2)
    X, _ = G.basis()
    ref = X @ np.linalg.solve(X.T @ (A2 @ X), X.T @ b)
    assert np.linalg.norm(x0 - ref) <= n * EPS * kappa(A2) * np.linalg.norm(ref)
    G.update(np.linalg.solve(A2.toarray(), b))
    assert G.info()["size"] == 5
    check_invariants(G, A2)


def test_rank_deficient_basis_after_a_matrix_change_is_cut():
    """Two directions orthonormal under A1 = I that A2 = I + 1000 z z^T, z = (q1 + q2) / sqrt 2, all but merges: with
    tol_dep = 0.5 the second Cholesky pivot, 501 - 500^2 / 501 = 2.0, is below 0.25 x 501 and the direction is dropped."""
    n = 50
    q1, q2, q3 = np.zeros(n), np.zeros(n), np.zeros(n)
    q1[3], q2[17], q3[30] = 1.0, 1.0, 1.0
    G = R.Guess(sp.identity(n, format="csr"), depth=4, tol_dep=0.5)
    G.update(2.0 * q1)
    G.update(2.0 * q1 + 2.0 * q2)                    # s = 4 > 0.25 x 8
    G.update(q1 + q2 + 3.0 * q3)
    assert G.info()["size"] == 3
    z = (q1 + q2) / np.sqrt(2.0)
    A2 = sp.csr_matrix(np.eye(n) + 1000.0 * np.outer(z, z))
    G.set_matrix(A2)
    G.project(np.ones(n))
    info = G.info()
    assert info["size"] == 1 and info["dropped"] == 2 and info["reorthonormalisations"] == 1
    check_invariants(G, A2)


def test_refusals():
    A = random_spd(50, 5)
    for depth in (0, 33):
        with pytest.raises(ValueError):
            R.Guess(A, depth=depth)
    with pytest.raises(ValueError):
        R.Guess(A, tol_dep=0.0)
    G = R.Guess(A)
    G.update(np.ones(50))
    before = G.basis()
    bad = np.ones(50)
    bad[7] = np.nan
    with pytest.raises(ValueError):
        G.project(bad)
    with pytest.raises(ValueError):
        G.update(bad)
    with pytest.raises(ValueError):
        G.project(np.ones(49))
    assert np.array_equal(before[0], G.basis()[0]) and G.info()["size"] == 1


def test_bindings_declare_the_guess_symbols():
    from deeppreconditioning_amd import _lib
    for name in ("create", "project", "update", "reset", "info", "get_basis", "destroy"):
        assert f"dpcg_guess_{name}" in _lib.SIGNATURES
