"""The preconditioned Lanczos process of csrc/dpcg_lanczos.hip (dpcg_spectrum, `CsrSystem.spectrum_bounds`) restated in numpy,
step by step.

Not a test.  `lanczos` follows the head comment of dpcg_lanczos.hip and makes the device's decisions by the device's rules:
  start:  v_i = hash(seed, i) (`_hash`: k_lz_start); u = M v; s = <v, u>; a non-finite s or s <= 0 ends the run at 0 steps;
          r_0 = v / sqrt(s), z_0 = u / sqrt(s).
  step j: w = A z_j; alpha_j = <z_j, w>; w = (w - alpha_j r_j) - beta_j r_{j-1} (beta_0 = 0); classical Gram-Schmidt twice over
          the columns 0..j: c_i = <z_i, w>, w -= sum_i c_i r_i (columns ascending from zero, one product and one addition per
          column, as k_lz_update does); u = M w; s = <w, u> (k_lz_fin_beta): non-finite -> NONFINITE; s > 0 -> beta_{j+1} =
          sqrt(s), r_{j+1} = w / beta_{j+1}, z_{j+1} = u / beta_{j+1}; -s <= 1e-13 (alpha_j^2 + beta_j^2) -> INVARIANT with
          beta_{j+1} = 0; otherwise NOT_SPD.  Each of the three ends the run with `steps` = j + 1.
Only the inner products over the rows have a free order, chosen by `sums`: "sequential" (first row to last) or "pairwise" (numpy's
blocked pairwise sum) -- two legitimate orders; the device (per-wave partials, then one fixed order) is a third, and the distance
between the two is the yardstick of tests/test_spectrum_edges_gpu.py, as in tests/guess_restatement.py.  A z is scipy's CSR
product: each row's products added in column order, which is the order of the device's SpMV.
Every product and every addition is rounded on its own here; so it is on the device, because csrc/Makefile builds libdpcg.so with
-ffp-contract=off (hipcc would otherwise fuse `x - al * r` and `acc + ci * r`).  The n <= 3 cases of the edge tests, where the device
has to give the restatement's bits, rest on that flag.
"""

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

RUNNING, INVARIANT, NOT_SPD, NONFINITE = "running", "invariant", "not SPD", "non-finite"
MASK64 = (1 << 64) - 1


def _hash(seed, idx):
    """The start vector's counter-based hash (k_lz_start) restated in numpy: splitmix64's finaliser of a counter."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + (idx.astype(np.uint64) + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) * 2.0 - 1.0


def hash_scalar(seed, i):
    """`_hash` for one (seed, index) in Python integers, every product reduced mod 2^64 by hand: what lz_hash computes."""
    x = ((seed & MASK64) * 0x9E3779B97F4A7C15 + ((i + 1) & MASK64) * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return float(x >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0


def _lanczos_numpy(A, Mdense_apply, seed, k):
    """fp64 restatement of the recurrence of dpcg_lanczos.hip (M inner product, CGS2) with numpy's own matrix products: the
    reference of tests/test_spectrum_gpu.py::test_first_steps_match_numpy, kept as it was.  `lanczos` below is the one that
    fixes every order and makes the device's decisions."""
    n = A.shape[0]
    v = _hash(seed, np.arange(n))
    u = Mdense_apply(v)
    nrm = np.sqrt(v @ u)
    R, Z = [v / nrm], [u / nrm]
    alpha, beta = [], [0.0]
    for j in range(k):
        w = A @ Z[j]
        a = Z[j] @ w
        w = w - a * R[j]
        if j > 0:
            w = w - beta[j] * R[j - 1]
        for _ in range(2):
            Rm, Zm = np.array(R).T, np.array(Z).T
            w = w - Rm @ (Zm.T @ w)
        u = Mdense_apply(w)
        b = np.sqrt(w @ u)
        alpha.append(a)
        beta.append(b)
        R.append(w / b)
        Z.append(u / b)
    return np.array(alpha), np.array(beta[1:])


def _dot(a, b, sums):
    p = a * b
    return float(np.cumsum(p, out=p)[-1]) if sums == "sequential" else float(np.sum(p))


@dataclass
class LanczosRun:
    """alpha[:steps] and beta (beta[i] = beta_{i+1} of T, the coupling after step i + 1, as `SpectrumBounds.beta`): `steps` entries
    when the run is RUNNING or INVARIANT (the last is then 0), steps - 1 when it ended NOT_SPD or NONFINITE at step `steps`.
    `s` is the last <w, M w> and `scale` the alpha_j^2 + beta_j^2 it was judged against (0 at the start vector); `s_min_ratio` is the
    smallest s / scale over the steps that went on, i.e. how far every accepted step stayed from the decision."""
    alpha: np.ndarray
    beta: np.ndarray
    status: str
    steps: int
    s: float
    scale: float
    s_min_ratio: float


def lanczos(A, M_apply, seed, k, sums="sequential"):
    """At most k <= n steps from the start vector of `seed`; see the module's docstring."""
    assert sums in ("sequential", "pairwise")
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    assert 1 <= k <= n
    alpha, beta = [], []

    def result(status, steps, s, scale, ratio):
        return LanczosRun(np.array(alpha), np.array(beta), status, steps, s, scale, ratio)

    v = _hash(seed, np.arange(n))
    u = np.asarray(M_apply(v), dtype=np.float64)
    s = _dot(v, u, sums)
    if not np.isfinite(s):
        return result(NONFINITE, 0, s, 0.0, np.inf)
    if not s > 0.0:
        return result(NOT_SPD, 0, s, 0.0, np.inf)
    norm0 = np.sqrt(s)
    R, Z = [v / norm0], [u / norm0]
    b_prev = 0.0
    ratio = np.inf
    for j in range(k):
        w = A @ Z[j]
        a = _dot(Z[j], w, sums)
        alpha.append(a)
        w = w - a * R[j]
        if j > 0:
            w = w - b_prev * R[j - 1]
        for _ in range(2):
            c = [_dot(Z[i], w, sums) for i in range(j + 1)]
            acc = np.zeros(n)
            for i in range(j + 1):
                acc = acc + c[i] * R[i]
            w = w - acc
        u = np.asarray(M_apply(w), dtype=np.float64)
        s = _dot(w, u, sums)
        scale = a * a + b_prev * b_prev
        if not np.isfinite(s):
            return result(NONFINITE, j + 1, s, scale, ratio)
        if not s > 0.0:
            if -s <= 1e-13 * scale:
                beta.append(0.0)
                return result(INVARIANT, j + 1, s, scale, ratio)
            return result(NOT_SPD, j + 1, s, scale, ratio)
        ratio = min(ratio, s / scale)
        b_prev = np.sqrt(s)
        beta.append(b_prev)
        R.append(w / b_prev)
        Z.append(u / b_prev)
    return result(RUNNING, k, s, scale, ratio)


def ritz_values(alpha, beta):
    """Eigenvalues of T_k = tridiag(beta[:k-1], alpha, beta[:k-1]), ascending, k = len(alpha)."""
    k = len(alpha)
    T = np.diag(np.asarray(alpha, dtype=np.float64))
    if k > 1:
        off = np.asarray(beta, dtype=np.float64)[: k - 1]
        T = T + np.diag(off, 1) + np.diag(off, -1)
    return np.linalg.eigvalsh(T)


def spectrum_distance(theta, lam):
    """max_i |theta_i - lam_i| / max |lam|: the distance of two whole spectra, relative to the largest eigenvalue (the scale to
    which a symmetric eigenvalue routine resolves every eigenvalue)."""
    theta, lam = np.sort(np.asarray(theta)), np.sort(np.asarray(lam))
    assert theta.shape == lam.shape
    return float(np.max(np.abs(theta - lam)) / np.max(np.abs(lam)))


def jacobi_similar_eigs(A, dinv=None):
    """Eigenvalues of M A for M = diag(dinv) (None: M = I) from the symmetric D^-1/2 A D^-1/2."""
    Ad = sp.csr_matrix(A).toarray()
    if dinv is not None:
        h = np.sqrt(dinv)
        Ad = h[:, None] * Ad * h[None, :]
    return np.linalg.eigvalsh(Ad)


def sequence_distance(x, y):
    """max_j |x_j - y_j| / |y_j|: the largest relative distance over the steps of a case (0 where both are the same bits)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape
    if y.size == 0:
        return 0.0
    d = np.abs(x - y)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / np.abs(y))))
