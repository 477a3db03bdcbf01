"""tests/spectrum_restatement.py checked on its own (CPU): the restated Lanczos process is the yardstick of
tests/test_spectrum_edges_gpu.py only if it is right.

eps = 2^-53.  Bound of the whole-spectrum test: n steps of a fully reorthogonalised Lanczos process give T_n = Z^T A Z with an
M-orthonormal basis up to O(eps) per step, so T_n is the projection of a matrix within c n eps ||M A|| of M A, and eigvalsh
resolves both spectra to n eps of the largest eigenvalue: |theta_i - lambda_i| <= 4 n eps lambda_max with c = 2 for the process
and 1 for each eigvalsh.
"""

import numpy as np
import pytest
import scipy.sparse as sp

import spectrum_restatement as R
from oracle import oracle as O
from test_guess_gpu import tridiagonal

EPS = 2.0 ** -53
SIZES = (1, 2, 3, 63, 64, 65)


def m_apply(kind, A):
    if kind == "identity":
        return None, (lambda v: v.copy())
    dinv = 1.0 / A.diagonal()
    return dinv, (lambda v: dinv * v)


@pytest.mark.parametrize("kind", ["identity", "jacobi"])
@pytest.mark.parametrize("n", SIZES)
def test_whole_spectrum(n, kind):
    """k = n: the eigenvalues of T_n are those of D^-1/2 A D^-1/2 (of A for M = I).  Recorded: the largest distance, relative to
    lambda_max, over the twelve cases and both sum orders is 1.574e-15 (Jacobi, n = 65, pairwise; 14 eps), against the bound
    4 n eps = 2.9e-14 there; n = 1: 0; n = 2: 1.6e-16; n = 3: 6.3e-16; n = 63 .. 65: 6.1e-16 .. 1.6e-15.  The run ends INVARIANT
    (the last <w, M w> is exactly 0) at n = 1 and at n = 2 with Jacobi, and RUNNING with a last beta of 1e-49 .. 1e-46 elsewhere:
    w is reorthogonalised twice against a basis of the whole space, each pass leaving eps of what it found."""
    A = tridiagonal(n)
    dinv, M = m_apply(kind, A)
    lam = R.jacobi_similar_eigs(A, dinv)
    for sums in ("sequential", "pairwise"):
        run = R.lanczos(A, M, 0, n, sums)
        assert run.steps == n and run.status in (R.RUNNING, R.INVARIANT)
        assert len(run.alpha) == len(run.beta) == n
        d = R.spectrum_distance(R.ritz_values(run.alpha, run.beta), lam)
        print(f"n {n} {kind} {sums}: {run.status}, last beta {run.beta[-1]:.3e}, spectrum distance {d:.3e} bound {4 * n * EPS:.3e}")
        assert d <= 4 * n * EPS
        scale = np.sqrt(run.alpha[-1] ** 2 + (run.beta[-2] ** 2 if n > 1 else 0.0))
        assert 0.0 <= run.beta[-1] <= 1e-13 * scale
        if n == 1:
            assert run.status == R.INVARIANT and run.beta[-1] == 0.0


def test_first_steps_agree_with_the_matrix_form():
    """`lanczos` and `_lanczos_numpy` (BLAS products for the reorthogonalisation) are the same recurrence."""
    A = sp.csr_matrix(O.unstructured_like(O.poisson2d(32), 2))
    dinv = O.jacobi_dinv(A)
    a, b = R._lanczos_numpy(A, lambda v: dinv * v, 11, 10)
    for sums in ("sequential", "pairwise"):
        run = R.lanczos(A, lambda v: dinv * v, 11, 10, sums)
        assert run.status == R.RUNNING and run.steps == 10
        np.testing.assert_allclose(run.alpha, a, rtol=1e-12)
        np.testing.assert_allclose(run.beta, b, rtol=1e-12)


@pytest.mark.parametrize("seed,index", [(0, 0), (0, 1), (11, 1023), (2 ** 64 - 1, 0), (2 ** 64 - 1, 2 ** 32 + 5), (3, 2 ** 32),
                                        (0x123456789ABCDEF, 2 ** 40 + 12345)])
def test_hash_against_python_integers(seed, index):
    """The uint64 arithmetic of `_hash` wraps as Python integers reduced mod 2^64 do, also for the largest seed and for an index
    that does not fit 32 bits; the value lies in [-1, 1)."""
    got = R._hash(seed, np.array([index], dtype=np.uint64))[0]
    assert got == R.hash_scalar(seed, index)
    assert -1.0 <= got < 1.0
    assert got != R._hash(seed, np.array([index + 1], dtype=np.uint64))[0]


def test_hash_is_splitmix64():
    """With seed 0 and index i the state before the finaliser is (i + 1) 0xBF58476D1CE4E5B9; splitmix64's finaliser of the state 1,
    worked by hand in Python integers, is 0x5692161D100B05E5 (Steele, Lea & Flood 2014: x ^= x >> 30, * 0xBF58476D1CE4E5B9,
    x ^= x >> 27, * 0x94D049BB133111EB, x ^= x >> 31)."""
    x = 1
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) % 2 ** 64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) % 2 ** 64
    x ^= x >> 31
    assert x == 0x5692161D100B05E5
    inv = pow(0xBF58476D1CE4E5B9, -1, 2 ** 64)          # the index whose state is 1: (i + 1) = 0xBF58476D1CE4E5B9^-1 mod 2^64
    assert R.hash_scalar(0, inv - 1) == float(x >> 11) * 2.0 ** -53 * 2.0 - 1.0


def indefinite_case():
    """The 8 x 8 five-point Laplacian with M = diag(+1 on the first 48 rows, -1 on the last 16)."""
    A = sp.csr_matrix(O.poisson2d(8))
    m = np.concatenate([np.ones(48), -np.ones(16)])
    return A, m


@pytest.mark.parametrize("seed", [0, 5])
def test_indefinite_m_is_found_out(seed):
    """An indefinite M whose start product <v, M v> is positive ends NOT_SPD at a step k <= n.  It has to: while the run goes on,
    the columns r_0 .. r_j are M-orthonormal (<r_i, M r_j> = <r_i, z_j> = delta_ij), hence independent.  n of them are a basis of
    the whole space in which <x, M x> = sum c_i^2 > 0 for every x = sum c_i r_i != 0: M would be positive definite.  So an
    indefinite M cannot let n - 1 steps go on, let alone n (in exact arithmetic; an invariant space ends the run sooner still).
    Recorded: for every seed 0 .. 399 the restatement stops at k = 1 (this M makes the first w negative at once: <w, M w> =
    -0.60 (alpha_0^2 + beta_0^2) for seed 0, -0.42 for seed 5 -- twelve orders of magnitude from the invariance threshold of
    1e-13), with both sum orders; the start product is positive (48 of 64 rows count positive)."""
    A, m = indefinite_case()
    n = A.shape[0]
    v = R._hash(seed, np.arange(n))
    assert v @ (m * v) > 0.0
    runs = [R.lanczos(A, lambda x: m * x, seed, n, sums) for sums in ("sequential", "pairwise")]
    for run in runs:
        print(f"seed {seed}: {run.status} after {run.steps} steps, s / scale {run.s / run.scale:.3e}")
        assert run.status == R.NOT_SPD and 1 <= run.steps <= n
        assert len(run.alpha) == run.steps and len(run.beta) == run.steps - 1
        assert -run.s > 1e-3 * run.scale and run.s_min_ratio > 1e-3          # far from either decision at every step
    assert runs[0].steps == runs[1].steps == 1


def test_statuses():
    A = tridiagonal(5)
    bad = np.array([1.0, 1.0, np.inf, 1.0, 1.0])
    run = R.lanczos(A, lambda v: bad * v, 0, 5)
    assert run.status == R.NONFINITE and run.steps == 0 and len(run.alpha) == 0
    run = R.lanczos(A, lambda v: -v, 0, 5)
    assert run.status == R.NOT_SPD and run.steps == 0
    calls = []

    def nan_from_the_third_call(v):
        calls.append(1)
        out = v.copy()
        if len(calls) >= 3:
            out[1] = np.nan
        return out

    run = R.lanczos(A, nan_from_the_third_call, 0, 5)
    assert run.status == R.NONFINITE and run.steps == 2 and len(run.alpha) == 2 and len(run.beta) == 1
    B = sp.kron(sp.identity(4), sp.csr_matrix(np.diag([1.0, 2.0]))).tocsr()       # two eigenvalues: the space ends after 2 steps
    run = R.lanczos(B, lambda v: v.copy(), 0, 8)
    th = R.ritz_values(run.alpha[:2], run.beta[:2])
    assert run.steps >= 2 and run.beta[1] <= 1e-13 and np.allclose(th, [1.0, 2.0], rtol=1e-14)
