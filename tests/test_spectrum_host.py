"""dpcg_tridiag_ritz (the host half of dpcg_spectrum) against numpy.linalg.eigh -- no GPU needed."""

import numpy as np
import pytest

from deeppreconditioning_amd import _lib
from deeppreconditioning_amd.operators import tridiag_ritz


def _dense(alpha, beta):
    return np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)


def _lanczos_tridiag(eigs, k, rng):
    """T_k of a fully reorthogonalised Lanczos process on diag(eigs): a tridiagonal with the spectrum's clusters."""
    n = eigs.size
    Q = np.zeros((n, k + 1))
    q = rng.standard_normal(n)
    Q[:, 0] = q / np.linalg.norm(q)
    a, b = np.zeros(k), np.zeros(k)
    for j in range(k):
        w = eigs * Q[:, j]
        a[j] = Q[:, j] @ w
        for _ in range(2):
            w -= Q[:, : j + 1] @ (Q[:, : j + 1].T @ w)
        b[j] = np.linalg.norm(w)
        Q[:, j + 1] = w / b[j]
    return a, b[: k - 1]


def _cases():
    rng = np.random.default_rng(7)
    for k in (1, 2, 50, 500):
        yield f"random-{k}", rng.standard_normal(k), rng.standard_normal(k - 1)
    for k in (2, 50, 500):
        n = max(k, 3)
        centres = np.array([1.0, 4.0, 40.0])
        eigs = np.sort(np.concatenate([c + 1e-4 * np.arange(n // 3 + 1) for c in centres])[:n])
        a, b = _lanczos_tridiag(eigs, k, rng)
        yield f"clustered-{k}", a, b
    for k in (2, 50, 500):
        a, b = rng.uniform(1, 3, k), rng.uniform(-1, 1, k - 1)
        b[:: max(1, k // 5)] = 0.0                   # split into unreduced blocks
        yield f"split-{k}", a, b


@pytest.mark.parametrize("name,alpha,beta", list(_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_tridiag_ritz_matches_eigh(name, alpha, beta):
    theta, bottom = tridiag_ritz(alpha, beta)
    T = _dense(alpha, beta)
    lam, V = np.linalg.eigh(T)
    norm = max(np.abs(lam).max(), 1e-300)
    np.testing.assert_allclose(theta, lam, rtol=0, atol=1e-12 * norm)
    assert np.all(np.diff(theta) >= 0)
    ref = np.abs(V[-1, :])
    got = np.abs(bottom)
    # eigenvectors of (nearly) equal eigenvalues are only defined up to a rotation inside their space: compare the invariant
    # sum of squares over each such group, every isolated one entry by entry
    group = np.concatenate([[0], np.cumsum(np.diff(lam) > 1e-9 * norm)])
    for g in np.unique(group):
        sel = group == g
        if sel.sum() == 1:
            np.testing.assert_allclose(got[sel], ref[sel], rtol=0, atol=1e-10)
        else:
            np.testing.assert_allclose(np.sum(got[sel] ** 2), np.sum(ref[sel] ** 2), rtol=0, atol=1e-10)
    np.testing.assert_allclose(np.sum(bottom ** 2), 1.0, rtol=0, atol=1e-10)


def test_tridiag_ritz_rejects_bad_input():
    with pytest.raises(_lib.DpcgError):
        _lib.check(_lib.lib().dpcg_tridiag_ritz(0, None, None, None, None))
    with pytest.raises(ValueError):
        tridiag_ritz(np.ones(3), np.ones(1))
