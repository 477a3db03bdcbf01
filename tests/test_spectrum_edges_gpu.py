"""CsrSystem.spectrum_bounds (dpcg_spectrum, csrc/dpcg_lanczos.hip) at its edges: the 4-rows-per-lane kernels step by step, the
host read every 16 steps, sizes on both sides of the 1024-row padding and of a wave, a Krylov space that is the whole space or
ends early, refusals after the start vector, a reordered handle step by step and a stream of the caller's.

Yardstick of "device equals restatement" (tests/spectrum_restatement.py), as in tests/test_guess_gpu.py: the restatement runs
with sequential and with pairwise sums -- two legitimate orders of the same recurrence; the device (per-wave partials, then one
fixed order) is a third.  The bar of a case is 8 x the largest relative distance between those two runs over all steps of the
case, for alpha and for beta separately; a single step's distance is one draw of a rounding error and no yardstick by itself.
Where the two host orders give the same bits over the whole case (n <= 3) the bar is 0: the device has to give those bits.
Steps are compared at rtol = 0.0 so that no run stops early; reorder="none" unless a test says otherwise.
"""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spectrum_restatement as R
from oracle import oracle as O
from test_guess_gpu import tridiagonal
from test_spectrum_gpu import _precond

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SMALL = (1, 2, 3, 63, 64, 65)


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def identity(v):
    return v.copy()


def jacobi(A):
    dinv = 1.0 / A.diagonal()
    return lambda v: dinv * v


_RUNS = {}


def restated(key, A, M, seed, k):
    """Both restatement runs of a case (sequential, pairwise), computed once and left unchanged."""
    if key not in _RUNS:
        seq, pair = (R.lanczos(A, M, seed, k, sums) for sums in ("sequential", "pairwise"))
        assert seq.status == pair.status and seq.steps == pair.steps, "the two orders disagree about a decision"
        _RUNS[key] = (seq, pair)
    return _RUNS[key]


def compare(sb, seq, pair, label, compared=None):
    """alpha and beta[:compared] of the device against the sequential run under the yardstick; returns the two bars."""
    m = len(seq.beta) if compared is None else compared
    assert len(sb.alpha) == len(seq.alpha) and len(sb.beta) >= m
    bar_a = 8 * R.sequence_distance(pair.alpha, seq.alpha)
    bar_b = 8 * R.sequence_distance(pair.beta[:m], seq.beta[:m])
    got_a = R.sequence_distance(sb.alpha, seq.alpha)
    got_b = R.sequence_distance(sb.beta[:m], seq.beta[:m])
    print(f"{label}: alpha device-restatement {got_a:.3e} bar {bar_a:.3e} | beta {got_b:.3e} bar {bar_b:.3e}")
    assert got_a <= bar_a
    assert got_b <= bar_b
    return bar_a, bar_b


def spectrum(D, A, M, reorder="none", **kw):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(M)
    sb = S.spectrum_bounds(**kw)
    reordered = S.reordered
    S.close()
    return sb, reordered


WIDE = {"tri_2^19-1": lambda: tridiagonal(2 ** 19 - 1), "tri_2^19": lambda: tridiagonal(2 ** 19),
        "poisson2d_725": lambda: sp.csr_matrix(O.poisson2d(725))}


@pytest.mark.parametrize("shape", list(WIDE))
def test_wide_rows_step_by_step(D, shape):
    """18 steps with Jacobi around n = 2^19, where k_lz_update goes from one row per lane (8 columns in flight) to four (4 columns in
    flight): 2^19 - 1 is the last size of the 1-row path with one padding row, 2^19 the first of the 4-row path without padding,
    525 625 = 725^2 has 711 padding rows.  The 18 steps include the host reads at 16 and at 18.
    What this test sees: the three-term update (MODE 0), the 16-byte loads and stores of the 4-row path, the padding, alpha and
    beta across a host read.  What it cannot see: the partials of Z^T w.  18 ordinary steps lose so little orthogonality that alpha
    and beta stay within their bars with no reorthogonalisation at all -- with the remainder loop of k_lz_update removed and its
    partials read as 0, all three cases still pass (measured with such a build of the library: 4.608e-14 instead of 4.619e-14 at
    2^19).  test_restarts_keep_the_basis_orthogonal and test_krylov_space_ends_early at m = 174 763 are the tests of those
    partials on the 4-row path.
    Measured on an MI355X (device to sequential restatement, then the bar): 2^19 - 1: alpha 3.7e-14 / 2.9e-13, beta 2.9e-14 /
    2.3e-13; 2^19: alpha 4.6e-14 / 3.7e-13, beta 2.4e-14 / 1.9e-13; 725^2: alpha 6.5e-14 / 5.2e-13, beta 2.3e-14 / 1.8e-13 -- an
    eighth of the bar throughout: the device's sums are as good as the pairwise ones, the sequential run is the outlier."""
    A = WIDE[shape]()
    n = A.shape[0]
    assert (n >= 2 ** 19) == (shape != "tri_2^19-1") and (-n) % 1024 == {"tri_2^19-1": 1, "tri_2^19": 0, "poisson2d_725": 711}[shape]
    seq, pair = restated(("wide", shape), A, jacobi(A), 0, 18)
    assert seq.status == R.RUNNING
    sb, _ = spectrum(D, A, D.Jacobi(), max_steps=18, rtol=0.0)
    assert sb.steps == 18 and not sb.converged
    compare(sb, seq, pair, f"wide {shape}")


def dense_eigs(A, kind):
    return R.jacobi_similar_eigs(A, 1.0 / A.diagonal() if kind == "jacobi" else None)


def restatement_spectrum_error():
    """The largest distance between the spectrum of the restatement's own T_n and the dense eigenvalues over the small cases, both
    preconditioners and both sum orders (tests/test_spectrum_restatement_host.py records it: 1.574e-15)."""
    if "own" not in _RUNS:
        worst = 0.0
        for kind in ("identity", "jacobi"):
            for n in SMALL:
                A = tridiagonal(n)
                lam = dense_eigs(A, kind)
                for run in restated(("small", n, kind), A, identity if kind == "identity" else jacobi(A), 0, n):
                    worst = max(worst, R.spectrum_distance(R.ritz_values(run.alpha, run.beta), lam))
        _RUNS["own"] = worst
    return _RUNS["own"]


@pytest.mark.parametrize("kind", ["identity", "jacobi"])
@pytest.mark.parametrize("n", SMALL)
def test_small_whole_spectrum(D, n, kind):
    """max_steps = n: the Krylov space is the whole space, T_n has the spectrum of M A, and the last beta is rounding noise --
    either a tiny s > 0 or s <= 0 and LZ_INVARIANT; both have to end with steps == n.  n = 1 with M = I takes LZ_INVARIANT for
    certain: sqrt(v v) == |v| makes z = +-1 exactly, so w = a z - a z = 0 exactly.  Sizes on both sides of a wave (63, 65), and the
    1023 .. 961 padding rows of every vector.
    Measured on an MI355X.  n <= 3: the two host orders agree to the bit and the device gives those bits (alpha, beta, and the same
    branch: LZ_INVARIANT at n = 1 and at n = 2 with Jacobi, a last beta of 6.1e-48 / 6.8e-49 / 1.7e-48 otherwise).  n = 63 .. 65:
    alpha 1.0e-14 .. 6.5e-13 against bars of 7.3e-14 .. 6.8e-12, beta 6.9e-15 .. 8.8e-13 against 1.7e-13 .. 9.9e-12, at most 0.14
    of its bar (the later coefficients of a whole-space run are sensitive: the bars are wider than at 18 steps); the last beta
    is 2e-47 .. 9e-47, always the s > 0 branch.  Spectrum of the device's T_n against dense: 0 .. 1.33e-15 against 1.26e-14."""
    A = tridiagonal(n)
    seq, pair = restated(("small", n, kind), A, identity if kind == "identity" else jacobi(A), 0, n)
    sb, _ = spectrum(D, A, D.Identity() if kind == "identity" else D.Jacobi(), max_steps=n, rtol=0.0)
    assert sb.steps == n and sb.converged
    assert len(sb.alpha) == len(sb.beta) == n
    compare(sb, seq, pair, f"small n {n} {kind}", compared=n - 1)
    last = sb.beta[-1]
    scale = np.sqrt(sb.alpha[-1] ** 2 + (sb.beta[-2] ** 2 if n > 1 else 0.0))
    print(f"small n {n} {kind}: last beta {last:.3e} ({'LZ_INVARIANT' if last == 0.0 else 'a tiny s > 0'}; restatement: {seq.status}, "
          f"{seq.beta[-1]:.3e}), err_min {sb.err_min:.3e} err_max {sb.err_max:.3e}")
    assert np.isfinite(last) and 0.0 <= last <= 1e-13 * scale
    assert np.isfinite(sb.err_min) and np.isfinite(sb.err_max) and sb.err_min >= 0.0 and sb.err_max >= 0.0
    lam = dense_eigs(A, kind)
    got = R.spectrum_distance(R.ritz_values(sb.alpha, sb.beta), lam)
    bar = max(8 * restatement_spectrum_error(), n * EPS)
    print(f"small n {n} {kind}: spectrum of the device's T_n against dense {got:.3e} bar {bar:.3e}")
    assert got <= bar
    if n == 1:
        assert seq.status == R.INVARIANT
        assert last == 0.0 and sb.err_min == 0.0 and sb.err_max == 0.0


@pytest.mark.parametrize("n", [1023, 1024, 1025, 4097])
def test_padding_jacobi(D, n):
    """18 steps on both sides of the 1024-row padding of the basis (1, 0, 1023 and 1023 padding rows; one, one, two and five
    workgroups of the store kernel).
    Measured on an MI355X (device, then bar): alpha 2.1e-15 .. 4.6e-15 against 1.6e-14 .. 3.9e-14, beta 1.2e-15 .. 2.1e-15
    against 9.7e-15 .. 1.7e-14: 0.12 .. 0.14 of the bar."""
    A = tridiagonal(n)
    seq, pair = restated(("pad", n), A, jacobi(A), 0, 18)
    sb, _ = spectrum(D, A, D.Jacobi(), max_steps=18, rtol=0.0)
    assert sb.steps == 18 and not sb.converged
    compare(sb, seq, pair, f"padding n {n} jacobi")


def test_padding_llt_multiply(D):
    """M = L L^T applied as L (L^T r) at n = 1025: the two triangular products have to leave the padding rows of u alone.  L is
    the random lower factor of tests/test_spectrum_gpu.py.
    Measured on an MI355X: alpha 2.7e-15 against a bar of 2.1e-14, beta 1.3e-15 against 8.9e-15."""
    n = 1025
    A = tridiagonal(n)
    pc = _precond(D, "llt-random", A)
    assert isinstance(pc, D.LLtMultiply)
    Lf = sp.csr_matrix((pc.val, pc.col, pc.rowptr), shape=(n, n))
    Lt = sp.csr_matrix(Lf.T)
    seq, pair = restated(("pad", "llt"), A, lambda r: Lf @ (Lt @ r), 0, 18)
    sb, _ = spectrum(D, A, pc, max_steps=18, rtol=0.0)
    assert sb.steps == 18 and not sb.converged
    compare(sb, seq, pair, "padding n 1025 LLtMultiply")


def test_reordered_handle_step_by_step(D):
    """The start vector is hashed from the caller's row index, so a handle that iterates in reverse Cuthill-McKee order walks through
    the alpha and beta of one that does not, and of the restatement in the caller's numbering -- for either seed; the seeds give
    different alpha.
    Measured on an MI355X: against the restatement alpha 4.4e-15 .. 5.9e-15 (bars 3.7e-14, 4.6e-14), beta 1.9e-15 .. 2.4e-15
    (bars 1.5e-14, 1.9e-14); rcm against none alpha 3.4e-16 and 6.8e-16, beta 2.2e-16 and 2.3e-16."""
    A = sp.csr_matrix(O.unstructured_like(O.poisson2d(64), 4))
    first = {}
    for seed in (0, 11):
        seq, pair = restated(("reorder", seed), A, jacobi(A), seed, 18)
        rcm, reordered = spectrum(D, A, D.Jacobi(), reorder="rcm", max_steps=18, rtol=0.0, seed=seed)
        assert reordered
        plain, reordered = spectrum(D, A, D.Jacobi(), reorder="none", max_steps=18, rtol=0.0, seed=seed)
        assert not reordered
        for sb in (rcm, plain):
            assert sb.steps == 18 and not sb.converged
        bar_a, bar_b = compare(rcm, seq, pair, f"reordered seed {seed} rcm")
        compare(plain, seq, pair, f"reordered seed {seed} none")
        got_a, got_b = R.sequence_distance(rcm.alpha, plain.alpha), R.sequence_distance(rcm.beta, plain.beta)
        print(f"reordered seed {seed}: rcm against none alpha {got_a:.3e} beta {got_b:.3e}")
        assert got_a <= bar_a and got_b <= bar_b
        first[seed] = plain.alpha
    assert R.sequence_distance(first[0], first[11]) > 1e-3


KRON_B = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])      # eigenvalues 3 - sqrt(3), 3, 3 + sqrt(3)


@pytest.mark.parametrize("m", [400, 174763])
def test_krylov_space_ends_early(D, m):
    """A = kron(I_m, B) has three eigenvalues (1.268, 3, 4.732), so every Krylov space ends after three steps: beta_4 is rounding
    noise.  Either the process stops there (s <= 0: LZ_INVARIANT, steps == 3) or a tiny s > 0 starts it again from a normalised
    rounding error, which ends after three steps likewise; the host read at 16 steps finds the extremes converged either way.
    The restatement takes the second way: beta = 1.4, 1.0, 6e-16, 1.6, 0.6, 9e-16, ... and T_16 holds each of B's extremes five
    times over.  m = 174 763 (n = 524 289, 1023 padding rows) is the same matrix on the 4-rows-per-lane kernels; it needs their
    reorthogonalisation to be right, because the restarted vector is rounding noise with a component of about n^-1/2 along every
    earlier column, which only Z^T w removes.  Measured with a build of the library whose k_lz_update has no remainder loop: both
    sizes fail here (no convergence; a non-finite <w, M w> after 61 and 71 steps).
    Measured on an MI355X, m = 400: the device takes the second way as well, steps == 16, converged, beta_4 = 5.9e-16; lambda_min is
    off by 8.9e-16 and lambda_max by 1.8e-15 against a bar of 5.0e-14; err_min 5e-40, err_max 1.8e-16.  m = 174 763: the second way again, steps == 16,
    converged, beta_4 = 5.8e-16, beta_5 = 1.64 (the space starts again); lambda_min off by 6.7e-16 and lambda_max by 8.9e-16 against
    a bar of 4.2e-13 (the sequential restatement itself is off by 5.2e-14 at this size); err_min 0, err_max 1.4e-16."""
    lam = np.linalg.eigvalsh(KRON_B)
    print("eigenvalues of B", lam)
    assert np.allclose(lam, [3 - np.sqrt(3), 3, 3 + np.sqrt(3)], rtol=1e-14)
    A = sp.kron(sp.identity(m), sp.csr_matrix(KRON_B)).tocsr()
    A.sort_indices()
    own = 0.0
    for run in restated(("kron", m), A, identity, 0, 16):
        th = R.ritz_values(run.alpha, run.beta)
        own = max(own, abs(th[0] - lam[0]), abs(th[-1] - lam[-1]))
    sb, _ = spectrum(D, A, D.Identity())
    bar = max(8 * own, 4 * EPS * lam[-1])
    print(f"kron m {m}: steps {sb.steps} converged {sb.converged} beta {sb.beta}")
    print(f"kron m {m}: lambda_min off by {abs(sb.lambda_min - lam[0]):.3e} lambda_max by {abs(sb.lambda_max - lam[-1]):.3e} bar {bar:.3e}"
          f" err_min {sb.err_min:.3e} err_max {sb.err_max:.3e}")
    assert sb.converged and sb.steps <= 16
    assert abs(sb.lambda_min - lam[0]) <= bar and abs(sb.lambda_max - lam[-1]) <= bar
    assert np.isfinite(sb.err_min) and np.isfinite(sb.err_max) and sb.err_min >= 0.0 and sb.err_max >= 0.0


@pytest.mark.parametrize("m", [400, 174763])
def test_restarts_keep_the_basis_orthogonal(D, m):
    """The matrix of test_krylov_space_ends_early, 18 steps at rtol = 0.0: six Krylov spaces of three steps each, every restart from
    rounding noise that has a component of about n^-1/2 along each earlier column.  Only the partials of Z^T w take those out, those
    of the remainder columns included, and then T_18 is six copies of B's spectrum coupled by beta of 1e-15: its 18 eigenvalues are
    B's three, six times each.  The start of a restart is one draw of a rounding error, so alpha and beta themselves have no bar
    worth the name here (the two host orders differ by 1e-3 after the first restart); the spectrum does.  Bar: 8 x the largest
    distance the restatement's own T_18 reaches (both sum orders), relative to lambda_max, with a floor of 4 eps.  Should the device
    end a space with s <= 0 (LZ_INVARIANT) it stops at a multiple of three steps and the same holds for fewer copies.
    The restatement with c = 0 for the remainder columns of k_lz_update (columns from 4 floor((j + 1) / 4) on) gives a distance of
    1e5 at either size, so this is the test that sees a wrong remainder column or partial on both paths; m = 174 763 (n = 524 289,
    1023 padding rows) is on the 4-rows-per-lane kernels.
    Measured on an MI355X: steps == 18 at both sizes, beta_4 = 5.9e-16 (m = 400) and 5.8e-16 (m = 174 763), the spectrum of T_18 is
    3.8e-16 from B's at both against bars of 1.9e-14 and 2.8e-13.  With a build of the library whose k_lz_update has no remainder
    loop (a scratch copy, run once on the MI355X) both sizes fail: the partials that are never written held stale memory in that
    run and the distance was 1e19; had they read as 0 the restatement above says 1e5."""
    lam = np.linalg.eigvalsh(KRON_B)
    A = sp.kron(sp.identity(m), sp.csr_matrix(KRON_B)).tocsr()
    A.sort_indices()
    own = 0.0
    for run in restated(("kron18", m), A, identity, 0, 18):
        assert run.steps == 18
        own = max(own, R.spectrum_distance(R.ritz_values(run.alpha, run.beta), np.repeat(lam, 6)))
    sb, _ = spectrum(D, A, D.Identity(), max_steps=18, rtol=0.0)
    print(f"restarts m {m}: steps {sb.steps} converged {sb.converged} beta {sb.beta}")
    assert sb.steps in (3, 6, 9, 12, 15, 18) and sb.converged == (sb.steps < 18)
    got = R.spectrum_distance(R.ritz_values(sb.alpha, sb.beta), np.repeat(lam, sb.steps // 3))
    bar = max(8 * own, 4 * EPS)
    print(f"restarts m {m}: spectrum of the device's T_{sb.steps} against B's, {sb.steps // 3} times each: {got:.3e} bar {bar:.3e}")
    assert got <= bar
    assert sb.beta[2] <= 1e-13 * np.sqrt(sb.alpha[2] ** 2 + sb.beta[1] ** 2)


def solve_and_spectrum(S, D, b):
    S.set_preconditioner(D.Jacobi())
    r = S.solve(b)
    return r, S.spectrum_bounds(seed=3)


def assert_same_bits(one, two):
    (r1, s1), (r2, s2) = one, two
    assert torch.equal(r1.x, r2.x) and np.array_equal(r1.res_history, r2.res_history) and r1.iterations == r2.iterations
    assert s1.alpha.tobytes() == s2.alpha.tobytes() and s1.beta.tobytes() == s2.beta.tobytes()
    assert s1.lambda_min == s2.lambda_min and s1.lambda_max == s2.lambda_max and s1.steps == s2.steps


@pytest.fixture(scope="module")
def fresh_64(D):
    """Solve and spectrum of the 8 x 8 Laplacian with Jacobi on a handle that never failed."""
    A = O.poisson2d(8)
    b = torch.from_numpy(O.rhs(64, 0)).cuda()
    S = D.CsrSystem.from_any(A, reorder="none")
    out = solve_and_spectrum(S, D, b)
    S.close()
    return A, b, out


@pytest.mark.parametrize("seed", [0, 5])
def test_not_spd_after_the_start(D, fresh_64, seed):
    """M = diag(+1 on 48 rows, -1 on 16) passes the start vector (<v, M v> > 0) and is found out at step k = 1 of the restatement,
    with <w, M w> = -0.60 (seed 0) and -0.42 (seed 5) of the step's scale: nowhere near the invariance threshold.  The device sets
    the status at that step, runs the remaining kernels of 16 steps as no-ops, and reports `after 1 steps` at its first read."""
    A, b, fresh = fresh_64
    m = np.concatenate([np.ones(48), -np.ones(16)])
    v = R._hash(seed, np.arange(64))
    assert v @ (m * v) > 0.0
    seq, pair = restated(("indefinite", seed), sp.csr_matrix(A), lambda x: m * x, seed, 64)
    for run in (seq, pair):
        assert run.status == R.NOT_SPD and -run.s > 1e-3 * run.scale and run.s_min_ratio > 1e-3
    k = seq.steps
    assert 1 <= k <= 64
    S = D.CsrSystem.from_any(A, reorder="none")
    S.set_preconditioner(D.CsrPreconditioner(sp.diags(m, format="csr")))     # (a bare diagonal matrix would be attached as Jacobi)
    assert isinstance(S._precond, D.CsrPreconditioner)
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds(max_steps=64, rtol=0.0, seed=seed)
    print(f"indefinite seed {seed}: restatement k = {k}; device: {exc.value}")
    assert exc.value.status == D._lib.BREAKDOWN
    assert f"after {k} steps" in str(exc.value) and "<w, M w> <= 0" in str(exc.value)
    assert_same_bits(solve_and_spectrum(S, D, b), fresh)
    S.close()


def test_nonfinite_jacobi(D, fresh_64):
    """dpcg_set_precond_jacobi copies a caller's dinv without looking at it, so one inf entry is accepted at attach; the start
    product <v, M v> is then infinite and spectrum_bounds refuses at 0 steps."""
    A, b, fresh = fresh_64
    dinv = O.jacobi_dinv(A).copy()
    dinv[10] = np.inf
    assert R.lanczos(sp.csr_matrix(A), lambda v: dinv * v, 0, 64).status == R.NONFINITE
    S = D.CsrSystem.from_any(A, reorder="none")
    S.set_preconditioner(D.Jacobi(dinv))
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds(max_steps=64, rtol=0.0)
    print(f"non-finite dinv: {exc.value}")
    assert exc.value.status == D._lib.BREAKDOWN and "non-finite" in str(exc.value) and "after 0 steps" in str(exc.value)
    assert_same_bits(solve_and_spectrum(S, D, b), fresh)
    S.close()


class _NanFromTheThirdCall:
    """M = I until its third call (the start vector and step 1 pass), then a NaN in row 7."""

    def __init__(self):
        self.calls = 0

    def __matmul__(self, r):
        self.calls += 1
        z = r.clone()
        if self.calls >= 3:
            z[7] = float("nan")
        return z


def test_nonfinite_after_the_start(D, fresh_64):
    """A NaN that appears in M w at step 2: the status is set with stop = 2, later kernels return at once, and the first host read
    reports it."""
    A, b, fresh = fresh_64
    host = _NanFromTheThirdCall()
    run = R.lanczos(sp.csr_matrix(A), lambda v: (host @ torch.from_numpy(v)).numpy(), 0, 64)
    assert run.status == R.NONFINITE and run.steps == 2
    S = D.CsrSystem.from_any(A, reorder="none")
    S.set_preconditioner(D.OperatorPreconditioner(_NanFromTheThirdCall()))
    with pytest.raises(D._lib.DpcgError) as exc:
        S.spectrum_bounds(max_steps=64, rtol=0.0)
    print(f"NaN from the third call: {exc.value}")
    assert exc.value.status == D._lib.BREAKDOWN and "non-finite" in str(exc.value) and "after 2 steps" in str(exc.value)
    assert_same_bits(solve_and_spectrum(S, D, b), fresh)
    S.close()


def test_callers_stream(D):
    """Every launch of dpcg_spectrum takes the caller's stream: the same bits as on the default stream, and a solve issued on that
    stream right after (it shares apply_precond's scratch) gives the default stream's solve."""
    A = O.poisson2d(48)
    b = torch.from_numpy(O.rhs(A.shape[0], 0)).cuda()
    S = D.CsrSystem.from_any(A)
    S.set_preconditioner(D.IC0("solve"))
    s0 = S.spectrum_bounds(seed=3)
    r0 = S.solve(b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side and side != torch.cuda.default_stream()
        s1 = S.spectrum_bounds(seed=3)
        r1 = S.solve(b)
    side.synchronize()
    assert s0.converged and s1.converged and s0.steps == s1.steps
    assert s0.alpha.tobytes() == s1.alpha.tobytes() and s0.beta.tobytes() == s1.beta.tobytes()
    assert s0.lambda_min == s1.lambda_min and s0.lambda_max == s1.lambda_max
    assert torch.equal(r0.x, r1.x) and np.array_equal(r0.res_history, r1.res_history)
    S.close()
