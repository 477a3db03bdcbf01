"""The edge cases of the mixed-precision PCG (dpcg_solve_refined, dpcg_refine.hip) shared by tests/test_refine_edges_host.py (CPU),
tests/test_refine_edges_gpu.py and tools/refine_probe.py --edges.  numpy / scipy only.

Short runs.  `solve_refined(b, max_iter=t, rtol_sq=1e-30, inner_rtol_sq=1e-300)` from x0 = None is ONE inner solve of t updates and
returns x = sigma d, sigma = sqrt(<b,b>): no outer step repairs what a wrong inner kernel did, and from t = 2 on every row of
q = fl32(A32 p) has fed r, p and d.  The systems enter every lanes-per-row class of k_rf_spmv (`lanes_per_row` restates the rule of
ensure_refine), with odd and even row starts, rows of one entry, a row far longer than the mean, stored zeros, values that fp32
rounds coarsely, and every n % 4 from n = 1 on.

Units.  One fp32 ulp of ||x||_inf is taken both as a number, spacing(fl32(||x||_inf)), and where the rounding happens,
sigma spacing(fl32(||d||_inf)); `x_ulp` is the SMALLER of the two (they differ by the binade sigma moves ||d||_inf into, at most a
factor 2).  A residual-history entry is compared relatively; its floor is 2^-22: one flipped store of r_i moves r_i by at most
2^-23 |r_i|, and <r,r> by at most 2 * 2^-23 r_i^2 <= 2^-22 <r,r>.

Tolerances are MEASURED on the CPU (the restatement under the perturbations of `PERTURBATIONS`), never picked: the device may
differ from the restatement by twice the measured spread, at least by the floor (`X_TOL_ULPS`, `HIST_TOL` below).
"""

from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

import edge_matrices as E
import refine_restatement as R

f32 = np.float32
PRES = ("identity", "jacobi")
TS = (1, 2, 3)
SHORT = {"rtol_sq": 1e-30, "inner_rtol_sq": 1e-300}
HIST_FLOOR = 2.0 ** -22

SYSTEMS = {**{f"tiny({n})": functools.partial(E.tiny, n) for n in range(1, 9)},                 # n4 == 0 and every n % 4
           "poisson2d(9)": lambda: E.poisson2d(9),
           "banded_spd(130, 6, 3)": lambda: E.banded_spd(130, 6, 3),
           "banded_spd(203, 12, 2)": lambda: E.banded_spd(203, 12, 2),
           "banded_spd(259, 24, 4)": lambda: E.banded_spd(259, 24, 4),
           "banded_spd(301, 40, 1)": lambda: E.banded_spd(301, 40, 1),
           "hub(12, 97)": lambda: E.hub(12, 97),                                                 # one row of 98 entries among short ones
           "boundary_identity(12)": lambda: E.boundary_identity(12),                             # rows of one entry
           "with_stored_zeros(poisson2d(12))": lambda: E.with_stored_zeros(E.poisson2d(12)),
           "scaled_rows(banded_spd(130, 6, 3), -3, 3, 1)": lambda: E.scaled_rows(E.banded_spd(130, 6, 3), -3, 3, 1)}
# the lanes-per-row class the table of the issue gives each system (asserted by the host test)
TPR = {**{f"tiny({n})": 2 for n in range(1, 9)}, "poisson2d(9)": 4, "banded_spd(130, 6, 3)": 8, "banded_spd(203, 12, 2)": 16,
       "banded_spd(259, 24, 4)": 32, "banded_spd(301, 40, 1)": 64, "hub(12, 97)": 4, "boundary_identity(12)": 4,
       "with_stored_zeros(poisson2d(12))": 4, "scaled_rows(banded_spd(130, 6, 3), -3, 3, 1)": 8}
SHORT_CASES = [(name, pre, t) for name in SYSTEMS for pre in PRES for t in TS]


def lanes_per_row(A) -> int:
    """the rule of ensure_refine (dpcg_refine.hip): a lane takes two non-zeros per trip"""
    n = A.shape[0]
    mean = A.nnz / n if n > 0 else 1.0
    tpr = 2
    while tpr < 64 and 2 * tpr < mean:
        tpr *= 2
    return tpr


@functools.lru_cache(maxsize=None)
def system(name):
    """(A, b): b = default_rng(1).random(n); int32 CSR with sorted indices (do not modify)"""
    A = E.csr(SYSTEMS[name]())
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A, np.random.default_rng(1).random(A.shape[0])


# ---- the perturbations the tolerances are measured with (tools/refine_probe.py uses the same for its count margin) ----------------
PERTURBATIONS = ("dots back to front", "b (1 + 1e-16 u)", "b (1 + 1e-12 u)")


def perturbed(b, tag):
    """(b', reverse) of one perturbation"""
    if tag == "dots back to front":
        return b, True
    eps = {"b (1 + 1e-16 u)": 1e-16, "b (1 + 1e-12 u)": 1e-12}[tag]
    return b * (1.0 + eps * np.random.default_rng(7).uniform(-1.0, 1.0, b.shape[0])), False


def short_kwargs(t):
    return dict(max_iter=t, **SHORT)


@functools.lru_cache(maxsize=None)
def short_run(name, pre, t, tag=""):
    """the restatement's short run of a case, as it stands (tag "") or under one perturbation; shared, do not modify"""
    A, b = system(name)
    bp, reverse = perturbed(b, tag) if tag else (b, False)
    return R.solve_refined(A, bp, jacobi=pre == "jacobi", reverse=reverse, **short_kwargs(t))


def x_ulp(x, b) -> float:
    """one fp32 ulp of ||x||_inf, the smaller of its two readings (module docstring)"""
    sigma = float(np.sqrt(b @ b))
    top = float(np.max(np.abs(x)))
    return float(min(np.spacing(f32(top)), sigma * np.spacing(f32(top / sigma))))


def x_distance(x, ref, b) -> float:
    """max_i |x_i - ref_i| in fp32 ulps of ||ref||_inf; an entry that is not finite on one side only counts as infinitely far"""
    fin = np.isfinite(x) & np.isfinite(ref)
    if not np.array_equal(np.isfinite(x), np.isfinite(ref)) or not fin.any():
        return 0.0 if np.array_equal(x, ref, equal_nan=True) else np.inf
    return float(np.max(np.abs(x[fin] - ref[fin]))) / x_ulp(ref[fin], b)


def hist_distance(h, ref) -> float:
    """max over the entries 1 .. of |h - ref| / ref (entry 0 is the outer value and compared exactly elsewhere)"""
    h, ref = np.asarray(h)[1:], np.asarray(ref)[1:]
    if h.shape != ref.shape:
        return np.inf
    if h.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(h == ref, 0.0, np.abs(h - ref) / np.abs(ref))
    return float(np.max(np.where(np.isfinite(rel), rel, np.inf)))


def measure_spread(name, pre, t):
    """(x spread in ulps, relative history spread, same counts?) of the restatement under PERTURBATIONS"""
    _, b = system(name)
    base = short_run(name, pre, t)
    sx = sh = 0.0
    same = True
    for tag in PERTURBATIONS:
        run = short_run(name, pre, t, tag)
        same = same and (run["status"], run["iterations"], run["outer_steps"]) == (base["status"], base["iterations"], base["outer_steps"])
        sx = max(sx, x_distance(run["x"], base["x"], b))
        sh = max(sh, hist_distance(run["res_history"], base["res_history"]))
    return sx, sh, same


# The device may differ from the restatement by twice the measured spread, at least by the floor.  Every measured spread is far
# below half a floor (x: <= 1.2e-5 ulp, history: <= 1.4e-15, profiles/refine_edges.md -- the perturbations flip no fp32 rounding
# in runs this short), so the floors ARE the tolerances; the host test re-measures every case and asserts 2 * spread <= floor.
X_TOL_ULPS = 1.0
HIST_TOL = HIST_FLOOR


# ---- mutants: the restatement with ONE entry of A32 set to zero, what a row kernel that drops or misreads an entry computes --------
MUTANTS = ("last entry of the widest row", "first entry of a row with an odd start", "the unpaired entry of a row of odd length")


def mutant_position(A, which):
    """index into A.data of the entry a mutant zeroes, or None where the system has no such entry.  Only entries whose fp32 value is
    not zero qualify (a stored zero changes nothing).  The unpaired entry of a row of odd length is the one k_rf_spmv does not read as
    half of an aligned pair inside the row: the last entry when the row starts at an even position (read alone), the first when it
    starts at an odd one (read with the entry before the row, which is masked); the even start is preferred since the mutant before
    it covers odd starts."""
    ip = A.indptr.astype(np.int64)
    length = np.diff(ip)
    nz = A.data.astype(f32) != 0
    if which == MUTANTS[0]:
        for i in np.argsort(-length, kind="stable"):
            if length[i] and nz[ip[i + 1] - 1]:
                return int(ip[i + 1] - 1)
        return None
    if which == MUTANTS[1]:
        for i in np.flatnonzero((ip[:-1] % 2 == 1) & (length > 0)):
            if nz[ip[i]]:
                return int(ip[i])
        return None
    odd = length % 2 == 1
    for i in np.flatnonzero(odd & (ip[:-1] % 2 == 0)):
        if nz[ip[i + 1] - 1]:
            return int(ip[i + 1] - 1)
    for i in np.flatnonzero(odd & (ip[:-1] % 2 == 1)):
        if nz[ip[i]]:
            return int(ip[i])
    return None


def one_inner_solve(A, b, pre, t, zeroed=None):
    """x = sigma d of one inner solve of (at most) t updates from x0 = None, the quantities of the short run; `zeroed`: the index of
    the entry of A32 set to zero.  dinv32 comes from A itself: the mutant is a wrong SpMV, not another matrix."""
    A32 = R.rounded_matrix(A)
    if zeroed is not None:
        A32.data[zeroed] = 0.0
    dinv32 = (1.0 / A.diagonal()).astype(f32) if pre == "jacobi" else None
    sigma = np.sqrt(R._dot(b, b, False))
    k, d, hist = R.inner_pcg(A32, (b / sigma).astype(f32), dinv32, SHORT["inner_rtol_sq"], t)
    return sigma * d.astype(np.float64)


@functools.lru_cache(maxsize=None)
def mutant_factor(name, pre, t, which):
    """distance of a mutant from the true restatement over the device's tolerance (None where the system has no such entry)"""
    A, b = system(name)
    pos = mutant_position(A, which)
    if pos is None:
        return None
    return x_distance(one_inner_solve(A, b, pre, t, pos), one_inner_solve(A, b, pre, t), b) / X_TOL_ULPS


# (system, preconditioner): the mutant claim is not made (at most two; the measured factors stand in the host test)
MUTANT_EXCLUSIONS = {}


# ---- stops and degenerate inputs ---------------------------------------------------------------------------------------------------
STAGNATION_CANDIDATES = {"scaled_rows(poisson2d(12), -4, 4)": lambda: E.scaled_rows(E.poisson2d(12), -4, 4),
                         "jumping((16, 16), 4, 1e8)": lambda: E.jumping((16, 16), 4, 1e8),
                         "anisotropic2d(16, 1e-6)": lambda: E.anisotropic2d(16, 1e-6),
                         "anisotropic2d(16, 1e-7)": lambda: E.anisotropic2d(16, 1e-7)}
STAGNATION_CASE = "anisotropic2d(16, 1e-7)"       # the one that qualifies (test_refine_edges_host.py)


@functools.lru_cache(maxsize=None)
def stagnation_run(name):
    """(A, b, the restatement's run with M = I, rtol_sq 1e-30 and the default inner target)"""
    A = E.csr(STAGNATION_CANDIDATES[name]())
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    b = np.random.default_rng(1).random(A.shape[0])
    return A, b, R.solve_refined(A, b, rtol_sq=1e-30, max_iter=20000)


def qualifies_as_stagnation(run) -> bool:
    return (run["reason"] == "stagnated" and run["outer_steps"] >= 2 and len(run["outer_margins"]) > 0
            and min(run["outer_margins"]) >= 1.2 and stagnation_margin(run) >= 1.2)


def stagnation_margin(run) -> float:
    """rr / (0.25 rr_prev) of the stop itself (>= 1: the larger, the clearer)"""
    h = run["outer_history"]
    return float(h[-1] / (0.25 * h[-2])) if len(h) >= 2 else 0.0


SCALING_SYSTEM = "banded_spd(130, 6, 3)"
SCALINGS = [(60, 200), (60, -200), (-60, 200), (-60, -200)]     # (k, m): (2^k A, 2^m b)
SCALING_KW = dict(rtol_sq=1e-20, max_iter=2000)


@functools.lru_cache(maxsize=None)
def scaling_restated(pre):
    A, b = system(SCALING_SYSTEM)
    return R.solve_refined(A, b, jacobi=pre == "jacobi", **SCALING_KW)


# ---- stops (section "stops and degenerate inputs"): every case is (A, b, x0, preconditioner, keyword arguments) -------------------
STOP_SYSTEM = "poisson2d(9)"
ZERO_MATRIX = "1e-50 tiny(5)"


def x0_of(n):
    return np.random.default_rng(4).random(n)


def _stop_system(name):
    if name == ZERO_MATRIX:
        A = E.csr(1e-50 * E.tiny(5))
        A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
        return A, np.random.default_rng(1).random(5)
    return system(name)


@functools.lru_cache(maxsize=None)
def first_inner(name, pre, rtol_sq=1e-20):
    """(updates of the first inner solve of the default call, how clear of its target the LAST BUT ONE test was: a factor >= 1)"""
    A, b = system(name)
    A32 = R.rounded_matrix(A)
    dinv32 = (1.0 / A.diagonal()).astype(f32) if pre == "jacobi" else None
    sigma = np.sqrt(R._dot(b, b, False))
    target = max(1e-6, 0.25 * rtol_sq)
    k, d, hist = R.inner_pcg(A32, (b / sigma).astype(f32), dinv32, target, 1024)
    return k, float(min(hist[:-1]) / target)


@functools.lru_cache(maxsize=None)
def atol_sq_for_step(name, pre, step=2):
    """an atol_sq that stops the default call (rtol_sq out of reach) at outer step `step` through rr < atol_sq: the geometric mean
    of the <r,r> of that step and of the one before"""
    A, b = system(name)
    free = R.solve_refined(A, b, jacobi=pre == "jacobi", rtol_sq=1e-300, max_outer=step)
    h = free["outer_history"] * float(b @ b)
    return float(np.sqrt(h[step - 1] * h[step]))


def stop_cases():
    """name -> (system, b or a tag, x0?, preconditioner, keyword arguments of solve_refined)"""
    out = {}
    for pre in PRES:
        out[f"atol_sq {pre}"] = (STOP_SYSTEM, "b", False, pre, dict(rtol_sq=1e-300, atol_sq=atol_sq_for_step(STOP_SYSTEM, pre)))
        out[f"max_outer {pre}"] = (STOP_SYSTEM, "b", False, pre, dict(rtol_sq=1e-20, inner_rtol_sq=1e-2, max_outer=3))
        out[f"cap at the end of an inner solve {pre}"] = (STOP_SYSTEM, "b", False, pre,
                                                          dict(rtol_sq=1e-20, max_iter=first_inner(STOP_SYSTEM, pre)[0]))
        out[f"zero updates {pre}"] = (STOP_SYSTEM, "b", False, pre, dict(rtol_sq=1e-20, inner_rtol_sq=2.0))
        out[f"zero updates from x0 {pre}"] = (STOP_SYSTEM, "b", True, pre, dict(rtol_sq=1e-20, inner_rtol_sq=2.0))
    for x0 in (False, True):
        tag = " from x0" if x0 else ""
        out[f"b = 0, atol_sq = 0{tag}"] = (STOP_SYSTEM, "zero", x0, "jacobi", dict())
        out[f"b = 0, atol_sq > 0{tag}"] = (STOP_SYSTEM, "zero", x0, "jacobi", dict(atol_sq=1e-10))
        out[f"b = 0, max_iter = 0{tag}"] = (STOP_SYSTEM, "zero", x0, "jacobi", dict(max_iter=0))
        out[f"b with one NaN{tag}"] = (STOP_SYSTEM, "nan", x0, "identity", dict())
    out["fp32 rounds A to zero"] = (ZERO_MATRIX, "b", False, "identity", dict())
    return out


def stop_inputs(case):
    """(A, b, x0 or None, preconditioner, keyword arguments).  b = 0 from x0 takes x0 = 0 GIVEN (the residual is formed through the
    SpMV and is 0/0 again); a non-zero x0 with b = 0 is rr / 0 = inf, not 0/0, and is no breakdown."""
    name, btag, with_x0, pre, kw = stop_cases()[case]
    A, b = _stop_system(name)
    n = A.shape[0]
    if btag == "zero":
        b = np.zeros(n)
    elif btag == "nan":
        b = b.copy()
        b[n // 2] = np.nan
    x0 = None
    if with_x0:
        x0 = np.zeros(n) if btag == "zero" else x0_of(n)
    return A, b, x0, pre, kw


@functools.lru_cache(maxsize=None)
def stop_restated(case):
    """the restatement's prediction of a stop case; shared, do not modify"""
    A, b, x0, pre, kw = stop_inputs(case)
    return R.solve_refined(A, b, x0=x0, jacobi=pre == "jacobi", **kw)
