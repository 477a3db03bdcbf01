"""The cases of tests/test_driver_forms_preconditioned_gpu.py, kept apart from it so that their classification (count case or not,
tests/driver_restatement.py::classify) can be checked WITHOUT a GPU: tests/test_driver_forms_cases_host.py runs every case's
restatement with M from the setups' own restatements (fsai_restatement, ilut_restatement, oracle.icholt, amg_restatement); the GPU
test runs the same cases with M taken from the device handle.  Not a test.

Systems (the smallest at which each form is taken): 33x31 Poisson (1 023 rows, odd, below the one-workgroup kernel's 6 144 and below
the whole-chip triangular-solve form's 1 024), the seeded edge-weighted 32x32 Laplacian + 0.05 I (1 024 rows: the first size that
form is offered), unstructured_like(poisson2d(79), 2) (6 241 rows: the first size past the one-workgroup kernel, the whole-chip L L^T kernel's)
and unstructured_like(poisson2d(40), 3) (1 600 rows, scattered, for the "solve" modes and reorder="rcm").
"""

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import deflation_restatement as DR
import driver_restatement as R
from oracle import oracle as O

RTOL_SQ = 1e-8
CAP_RTOL_SQ = 1e-24            # the capped cases: a threshold no solve reaches before its cap
MULTIPLY_CAP = 40              # multiplying by an incomplete factor squares the condition number: such solves run into any cap

SYSTEMS = {
    "33x31": lambda: DR.poisson((33, 31)),
    "w32x32": lambda: DR.shifted_laplacian((32, 32), 3),
    "p79u": lambda: _canonical(O.unstructured_like(O.poisson2d(79), seed=2)),
    "p40u": lambda: _canonical(O.unstructured_like(O.poisson2d(40), seed=3)),
}
# the seed of b (and of everything drawn with it) is 1, except where another one gives a preconditioner its share of count cases:
# PCG with FSAI gains only ~1.2 per update on these systems, so most right-hand sides stop within 1.2 of the threshold
B_SEED = {("fsai", "33x31"): 4, ("fsai", "p79u"): 3}

# preconditioner -> (how the driver sees it, the systems it is run on, whether its solves are capped at MULTIPLY_CAP)
PCS = {
    "fsai": dict(kind="llt_multiply", capped=False, systems=("33x31", "w32x32", "p79u")),
    "icholt_multiply": dict(kind="llt_multiply", capped=True, systems=("33x31", "w32x32", "p79u")),
    "icholt_solve": dict(kind="llt_solve", capped=False, systems=("33x31", "w32x32", "p40u")),
    "ilut_multiply": dict(kind="lu_multiply", capped=True, systems=("33x31", "w32x32", "p40u")),
    # (M = (L U)^-1 of ILUT(1, 0.1) is not symmetric: PCG does not converge with it in the restatement either -- capped like the products)
    "ilut_solve": dict(kind="lu_solve", capped=True, systems=("33x31", "w32x32", "p40u")),
    "amg": dict(kind="amg", capped=False, systems=("33x31", "w32x32", "p79u")),
    "amg_gs": dict(kind="amg", capped=False, systems=("33x31", "p40u")),
    # (the fp32 cycle rounds its work vectors: its restatement is discontinuous in b, so only its first updates can be count cases)
    "amg_fp32": dict(kind="amg", capped=False, systems=("p40u",)),
}
# the share of count cases is taken per preconditioner: the three AMG configurations are one
GROUPS = {"fsai": ("fsai",), "icholt": ("icholt_multiply", "icholt_solve"), "ilut": ("ilut_multiply", "ilut_solve"),
          "amg": ("amg", "amg_gs", "amg_fp32")}
# atol_sq / <b,b> of the "atol" cases (rtol_sq = 0: the absolute test is the one that ends the solve).  1e-7 where PCG converges;
# 2e-7 with AMG (Jacobi), whose histories pass 1e-7 within 1.2 on all three systems.  The capped preconditioners never converge (their
# histories RISE after the first update or two), so theirs is a value the history does cross, from the restatement's own histories:
# ICholT multiplied falls to 0.88 .. 0.97 at update 1, ILUT multiplied to 1.1 .. 1.5 at update 1 -- the absolute test ends those after
# one update -- and with ILUT solved only the first entry, <z0,z0>/<b,b> = 0.20 .. 0.29, is ever that small: the first test ends it.
ATOL_REL = {"icholt_multiply": 1.2, "ilut_multiply": 2.0, "ilut_solve": 0.5, "amg": 2e-7}
REORDERED = {"p79u", "p40u"}   # the scattered systems are also run on a reorder="rcm" handle


def _canonical(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


_MAT, _SYS = {}, {}


def matrix(name):
    if name not in _MAT:
        _MAT[name] = SYSTEMS[name]()
    return _MAT[name]


def system(pc, name):
    """(A, b, x0, x_true), computed once: b = default_rng(seed).random(n), x0 = default_rng(seed + 100).random(n); x_true from a
    host sparse solve."""
    seed = B_SEED.get((pc, name), 1)
    if (name, seed) not in _SYS:
        A = matrix(name)
        n = A.shape[0]
        b = np.random.default_rng(seed).random(n)
        _SYS[(name, seed)] = (A, b, np.random.default_rng(seed + 100).random(n), spla.spsolve(A.tocsc(), b))
    return _SYS[(name, seed)]


def make_preconditioner(D, pc):
    """The harness's own parameters: ICholT(1, 0.1), ILUT(1, 0.1), FSAI(level=1), the default SmoothedAggregation."""
    return {"fsai": lambda: D.FSAI(level=1), "icholt_multiply": lambda: D.ICholT("multiply", 1, 0.1),
            "icholt_solve": lambda: D.ICholT("solve", 1, 0.1), "ilut_multiply": lambda: D.ILUT("multiply", 1, 0.1),
            "ilut_solve": lambda: D.ILUT("solve", 1, 0.1), "amg": lambda: D.SmoothedAggregation(),
            "amg_gs": lambda: D.SmoothedAggregation(smoother="gauss_seidel"),
            "amg_fp32": lambda: D.SmoothedAggregation(precision="fp32")}[pc]()


# ---- M r from factors (the device's, or the setups' restatements') --------------------------------------------------------------
def apply_llt_multiply(Lf):
    Lf = sp.csr_matrix(Lf)
    Lt = sp.csr_matrix(Lf.T)
    return lambda r: Lf @ (Lt @ r)


def apply_llt_solve(Lf):
    Lc, Ltc = sp.csr_matrix(Lf), sp.csr_matrix(sp.csr_matrix(Lf).T)
    return lambda r: spla.spsolve_triangular(Ltc, spla.spsolve_triangular(Lc, r, lower=True), lower=False)


def apply_lu_multiply(Lf, Uf):
    Lf, Uf = sp.csr_matrix(Lf), sp.csr_matrix(Uf)
    return lambda r: Lf @ (Uf @ r)


def apply_lu_solve(Lf, Uf):
    Lf, Uf = sp.csr_matrix(Lf), sp.csr_matrix(Uf)
    return lambda r: spla.spsolve_triangular(Uf, spla.spsolve_triangular(Lf, r, lower=True, unit_diagonal=True), lower=False)


def apply_amg(pc, H, smoothers=None):
    """The V-cycle of the restatements fed a hierarchy (amg_restatement.Hierarchy): Jacobi fp64, Gauss-Seidel (with the smoothers of
    amg_smoother_restatement.smoothers_for) or the fp32 cycle."""
    import amg_fp32_restatement as R32
    import amg_restatement as AR
    import amg_smoother_restatement as SR
    if pc == "amg_fp32":
        M = R32.VCycle32(H)
        return lambda r: M @ r
    if pc == "amg_gs":
        return lambda r: SR.vcycle(H, smoothers, r, 1)
    return lambda r: AR.vcycle(H, r)


_CPU_M = {}


def cpu_apply(pc, name):
    """M from the setups' restatements: the same factors as the device's bit for bit (ICholT, ILUT, FSAI), the same hierarchy up to
    the Lanczos estimate of rho (AMG) -- what the classification is checked with where there is no GPU."""
    key = (pc, name)
    if key not in _CPU_M:
        A = matrix(name)
        if pc == "fsai":
            import fsai_restatement as FR
            _CPU_M[key] = apply_llt_multiply(FR.fsai(A, level=1))
        elif pc.startswith("icholt"):
            Lf = _CPU_M.setdefault(("icholt_factor", name), O.icholt(A, 1, 0.1))
            _CPU_M[key] = apply_llt_multiply(Lf) if pc == "icholt_multiply" else apply_llt_solve(Lf)
        elif pc.startswith("ilut"):
            import ilut_restatement as IR
            Lf, Uf = _CPU_M.setdefault(("ilut_factor", name), IR.ilut(A, 1, 0.1))
            _CPU_M[key] = apply_lu_multiply(Lf, Uf) if pc == "ilut_multiply" else apply_lu_solve(Lf, Uf)
        else:
            import amg_restatement as AR
            import amg_smoother_restatement as SR
            H = _CPU_M.setdefault(("amg_hierarchy", name), AR.hierarchy(A))
            _CPU_M[key] = apply_amg(pc, H, SR.smoothers_for(H, SR.GAUSS_SEIDEL) if pc == "amg_gs" else None)
    return _CPU_M[key]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    pc: str
    system: str
    variant: str
    reorder: "str | None" = None

    @property
    def id(self):
        return f"{self.pc}-{self.system}-{self.variant}"


def variant_kw(variant, pc=None):
    """What a variant changes: flags (names of _lib constants), start vector, thresholds, cap."""
    v = dict(flags=(), x0=False, rtol_sq=RTOL_SQ, atol_rel=0.0, cap=None, mixed=False)
    if variant in ("launches", "x0_launches", "init_r_launches"):
        v["flags"] = ("NO_SMALL", "NO_TEAM")
    if variant in ("x0", "x0_rcm", "x0_launches"):
        v["x0"] = True
    if variant in ("init_r", "init_r_launches"):
        v["x0"] = True
        v["flags"] = v["flags"] + ("INIT_CHECK_R",)
    if variant == "atol":
        v.update(rtol_sq=0.0, atol_rel=ATOL_REL.get(pc, 1e-7))
    if variant == "mixed":
        v.update(mixed=True, flags=("SPMV_F32",))
    if variant.startswith("cap"):
        tail = variant[3:]
        if tail.endswith("L"):
            tail = tail[:-1]
            v["flags"] = ("NO_SMALL", "NO_TEAM")
        v.update(cap=int(tail), rtol_sq=CAP_RTOL_SQ, x0=True)
    return v


def caps_of(pc):
    """0, 1, and caps that end a replayed chunk one update early WHATEVER chunk Solve::start picks: 8 by default, 1024 / launches per
    update where a level-scheduled solve makes an update 129 launches or more (`many_launches`; the natural-order factors here have
    93 and 110 levels, and how many of them are merged into one launch is the library's business), rounded up to even under
    DPCG_NO_FUSE -- so any of 2 .. 8.  7, 15, 23 are one less than a multiple of 2, 4, 8 (23 also of 3 and 6), 14 of 3 and 5, 13 of 7.
    AMG: chunks of 2 -- every odd cap -- and solves that end sooner, hence the smaller caps."""
    return (0, 1, 3, 5, 7) if PCS[pc]["kind"] == "amg" else (0, 1, 7, 13, 14, 15, 23)


def cases_of(pc):
    if pc == "amg_fp32":
        return [Case(pc, "p40u", "plain"), Case(pc, "p40u", "x0_rcm", "rcm"), Case(pc, "p40u", "cap1"), Case(pc, "p40u", "cap3")]
    out = []
    for name in PCS[pc]["systems"]:
        # a one-launch form takes the default call.  (The whole-chip triangular-solve form refuses the ICholT(1, 0.1) factor on every
        # system here, dpcg_solve_chip.hip::ensure_chip_trsv: in the natural order of 33x31 and w32x32 it has 93 and 110 dependency levels
        # against the form's limit of 18; on p40u, 16 levels, but rows with fill of up to 13 entries, more than the slots beside A's row
        # -- so "solve" stays on the launches)
        one_launch = PCS[pc]["kind"] == "llt_multiply"
        out += [Case(pc, name, "plain"), Case(pc, name, "x0"), Case(pc, name, "init_r"), Case(pc, name, "atol")]
        if one_launch:
            out += [Case(pc, name, "launches"), Case(pc, name, "x0_launches"), Case(pc, name, "init_r_launches")]
        if name in REORDERED:
            out.append(Case(pc, name, "x0_rcm", "rcm"))
    first = PCS[pc]["systems"][0]
    last = PCS[pc]["systems"][-1]
    for cap in caps_of(pc):
        out.append(Case(pc, last, f"cap{cap}"))
        if PCS[pc]["kind"] == "llt_multiply":
            out.append(Case(pc, last, f"cap{cap}L"))
        # the first system too: every cap where its factor has the many levels (the "solve" modes in natural order), else two of them
        if first != last and (cap in (1, 7) or PCS[pc]["kind"] in ("llt_solve", "lu_solve")):
            out.append(Case(pc, first, f"cap{cap}"))
    return out


ALL_CASES = [c for pc in PCS for c in cases_of(pc)]


def solve_args(case):
    """(x0, rtol_sq, atol_sq, max_iter, init_check_r) of a case."""
    A, b, x0, _ = system(case.pc, case.system)
    v = variant_kw(case.variant, case.pc)
    cap = v["cap"] if v["cap"] is not None else (MULTIPLY_CAP if PCS[case.pc]["capped"] else 1024)
    return (x0 if v["x0"] else None, v["rtol_sq"], v["atol_rel"] * float(b @ b), cap, "INIT_CHECK_R" in v["flags"])


def reference(case, apply_m, b=None, x_true=None):
    """The restatement's solve of a case with the given M."""
    A, b0, _, _ = system(case.pc, case.system)
    x0, rtol_sq, atol_sq, cap, icr = solve_args(case)
    spmv = R.mixed_spmv(A) if variant_kw(case.variant, case.pc)["mixed"] else None
    return R.pcg(A, b0 if b is None else b, apply_m, x0=x0, rtol_sq=rtol_sq, atol_sq=atol_sq, max_iter=cap, init_check_r=icr, spmv=spmv,
                 x_true=x_true)


def classify(case, apply_m):
    """(reference, margin, moved, prefix) of a case."""
    A, b, _, _ = system(case.pc, case.system)
    _, rtol_sq, atol_sq, _, _ = solve_args(case)
    ref = reference(case, apply_m)
    margin, moved, prefix = R.classify(A, b, ref, lambda b2: reference(case, apply_m, b=b2), rtol_sq, atol_sq)
    return ref, margin, moved, prefix


# ---- the projected guess: three right-hand sides in sequence ------------------------------------------------------------------------
GUESS_SOLVES = 3


def guess_id(pc, i):
    return f"{pc}-{PCS[pc]['systems'][0]}-guess{i}"


class GuessRun:
    """The restatement's side of `solve(guess=)` on a preconditioner's first system: b, b + 0.05 d1, b + 0.05 d2 one after the other.
    The Guess of tests/guess_restatement.py is kept twice, with sequential and with pairwise sums -- the two legitimate orders whose
    distance is the yardstick of tests/test_guess_gpu.py -- and both are handed the solutions `feed` gives them: the device's own on
    the GPU (so that the start vector of solve i is the one the device has to form), the restatement's where there is none.
    With the fp32 V-cycle the three solves are never count cases, whatever one perturbation shows: the cycle rounds its vectors, and a
    rounding that falls the other way in another summation order is amplified over the solve, as with DPCG_SPMV_F32."""

    def __init__(self, pc, apply_m):
        import guess_restatement as GR
        self.pc, self.m = pc, apply_m
        self.A, b, _, _ = system(pc, PCS[pc]["systems"][0])
        rng = np.random.default_rng(12)
        d1, d2 = rng.random(b.size), rng.random(b.size)
        self.rhs = (b, b + 0.05 * d1, b + 0.05 * d2)
        self.cap = MULTIPLY_CAP if PCS[pc]["capped"] else 1024
        self.guesses = {sums: GR.Guess(self.A, depth=4, sums=sums) for sums in ("sequential", "pairwise")}
        self.dist_x0 = 0.0          # the largest distance of the two orders' x0 over the sequence so far, relative to |x0|

    def step(self, i):
        """(b_i, x0, reference, margin, moved, prefix) of solve i; x0 is the sequential order's."""
        bi = self.rhs[i]
        x0 = {sums: g.project(bi) for sums, g in self.guesses.items()}
        nx = np.linalg.norm(x0["sequential"])
        if nx > 0:
            self.dist_x0 = max(self.dist_x0, float(np.linalg.norm(x0["sequential"] - x0["pairwise"]) / nx))
        run = lambda b2: R.pcg(self.A, b2, self.m, x0=x0["sequential"], rtol_sq=RTOL_SQ, max_iter=self.cap)      # noqa: E731
        ref = run(bi)
        margin, moved, prefix = R.classify(self.A, bi, ref, run, RTOL_SQ)
        return bi, x0["sequential"], ref, margin, moved, prefix

    def feed(self, x):
        for g in self.guesses.values():
            g.update(x)


# The cases that are NOT count cases with the restatements' factors (tests/test_driver_forms_cases_host.py asserts the list, and that
# at least two thirds of every preconditioner's cases, and one per form, are count cases).  Every other case is a COUNT case: its stop
# margin is >= 1.2 and its history moves by less than 1e-11 under a 1e-16 perturbation of b, and the GPU test asserts both.  The three
# solves of every preconditioner's guess= sequence are named here as well (they stand outside the shares).
NOT_COUNT_CASES = frozenset({
    "fsai-33x31-x0",
    "fsai-33x31-init_r",
    "fsai-33x31-x0_launches",
    "fsai-33x31-init_r_launches",
    "fsai-w32x32-plain",
    "fsai-w32x32-atol",
    "fsai-w32x32-launches",
    "fsai-p79u-plain",
    "fsai-p79u-atol",
    "fsai-p79u-launches",
    "fsai-33x31-guess1",
    "fsai-33x31-guess2",
    "icholt_multiply-w32x32-plain",
    "icholt_multiply-w32x32-x0",
    "icholt_multiply-w32x32-init_r",
    "icholt_multiply-w32x32-launches",
    "icholt_multiply-w32x32-x0_launches",
    "icholt_multiply-w32x32-init_r_launches",
    "icholt_solve-p40u-plain",
    "icholt_solve-33x31-guess1",
    "amg_fp32-p40u-plain",
    "amg_fp32-p40u-x0_rcm",
    "amg_fp32-p40u-guess0",
    "amg_fp32-p40u-guess1",     # (stable under the one perturbation, but never held to the count rule: see GuessRun)
    "amg_fp32-p40u-guess2",
})
GUESS_IDS = frozenset(guess_id(pc, i) for pc in PCS for i in range(GUESS_SOLVES))
COUNT_CASES = (frozenset(c.id for c in ALL_CASES) | GUESS_IDS) - NOT_COUNT_CASES


_YARDSTICK = []


def guess_x0_yardstick():
    """The bar for a start vector formed by the device against the sequential restatement's, relative to |x0|: 8 x the largest distance
    between the sequential and the pairwise restatement (tests/test_guess_gpu.py: a single step's distance is one draw of a rounding
    error and no yardstick by itself, hence the largest) -- over the sequences of all the preconditioners here, run with the setups'
    restatements and the restatement's own solutions, so the bar is the same number with and without a GPU."""
    if not _YARDSTICK:
        worst = 0.0
        for pc in PCS:
            run = GuessRun(pc, cpu_apply(pc, PCS[pc]["systems"][0]))
            for i in range(GUESS_SOLVES):
                run.feed(run.step(i)[2].x)
            worst = max(worst, run.dist_x0)
        _YARDSTICK.append(8.0 * worst)
    return _YARDSTICK[0]
