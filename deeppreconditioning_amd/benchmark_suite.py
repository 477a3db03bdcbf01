"""`BenchmarkSuite` harness compatible with `uibk/deep_preconditioning/test.py:31-198`.

Same technique names, same result columns (`kappas,densities,iterations,setups,durations,totals,successes`,
test.py:180) and the same `table.csv` / `totals.csv` layout, but the systems stay sparse and on the GPU: no dense
N x N reconstruction (test.py:61-68), no dense `L @ L.T` (test.py:103-104).  Unlike the reference, result lists are
instance attributes and nothing is created at import time (test.py:50-59 does both at class definition).
"""

from __future__ import annotations

import pathlib
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from ._lib import BREAKDOWN, DpcgError
from .cg import preconditioned_conjugate_gradient
from .io import coo_to_csr_device
from .model import lower_factor_csr, tril_batch_from_csr
from .operators import FSAI, IC0, ICT, ILUT, ICholT, CsrSystem, Identity, Jacobi, LLtMultiply, SmoothedAggregation

PARAMETERS = ["kappas", "densities", "iterations", "setups", "durations", "totals", "successes"]  # test.py:180

# How far each technique's row of `table.csv` may be compared with the reference's own table (written to `comparability.csv`
# beside it).  `incomplete_cholesky` runs the reference's default, `ilupp.icholt(add_fill_in=1, threshold=0.1)` (test.py:81-88),
# as ILU++ describes the algorithm (dual-threshold ICT on the lower triangle; oracle.icholt / dpcg_set_precond_icholt): the
# ilupp binary is absent here (not vendored, no network), so the factor is pinned to the published description, not to
# ilupp's output -- the norm and the tie-break the papers leave open are stated in the contract.
COMPARABILITY = {
    "vanilla": "comparable: M = I (test.py:70-72)",
    "jacobi": "comparable: M = diag(1/a_ii) (test.py:74-79)",
    "incomplete_cholesky": "algorithm per ILU++'s description (dual-threshold ICT: drop below threshold * ||column||_2, keep the "
                           "nnz + add_fill_in largest), ilupp binary absent: values unpinned against ilupp itself",
    "incomplete_cholesky_level1": "not in the reference: this library's static-pattern ICT (level-1 fill + MATLAB's 'ict' drop rule)",
    "incomplete_cholesky_0": "algorithm comparable (textbook IC(0) = ilupp.ichol0's definition), values unpinned against ilupp",
    "incomplete_cholesky_solve": "not in the reference: IC(0) applied by triangular solves",
    "incomplete_cholesky_multicolor": "not in the reference: IC(0) of the system in multicolour order, applied by triangular solves "
                                      "(another elimination order: another preconditioner; the fastest of the IC variants here)",
    "learned": "comparable given the same checkpoint; spconv's weight layout is assumed KRSC (unpinned)",
    "algebraic_multigrid": "same family as pyamg's smoothed_aggregation_solver(A).aspreconditioner(cycle='V') (test.py:95-98): "
                           "symmetric strength, MIS(2) aggregation, Jacobi-smoothed prolongator, Galerkin levels, exact coarse solve; "
                           "smoothed by damped Jacobi instead of Gauss-Seidel; pyamg absent: unpinned; applied, not materialised",
    "algebraic_multigrid_gauss_seidel": "not in the reference: the algebraic_multigrid hierarchy smoothed by symmetric Gauss-Seidel in "
                                        "multicolour order (each colour at once; pyamg sweeps row by row: another operator); a level "
                                        "that needs more than 63 colours keeps damped Jacobi",
    "algebraic_multigrid_chebyshev": "not in the reference: the algebraic_multigrid hierarchy smoothed by a degree-2 Chebyshev "
                                     "polynomial in D^-1 A on [rho / 30, rho] (pyamg's default smoother is Gauss-Seidel)",
    "algebraic_multigrid_fp32": "not in the reference: the algebraic_multigrid hierarchy (built in fp64, the same bits) with the cycle's "
                                "operands and work vectors stored in fp32 and all arithmetic in fp64; PCG itself stays fp64",
    "incomplete_lu": "algorithm per Saad's dual-threshold ILUT(p, tau) as restated in tests/ilut_restatement.py (M = L U multiplied, "
                     "test.py:90-93); ilupp binary absent: values unpinned; ilupp.ilut's own default arguments cannot be read here, "
                     "icholt's (add_fill_in=1, threshold=0.1) are assumed",
    "sparse_approximate_inverse": "not in the reference: the factorised sparse approximate inverse (FSAI, Kolotilina & Yeremin 1993) on "
                                  "tril(A) -- the closed-form optimum of ||I - L^T U_A||_F on a fixed pattern, the untrained twin of "
                                  "`learned`; M = L L^T multiplied",
    "sparse_approximate_inverse_level2": "not in the reference: FSAI on the lower triangle of the pattern of A^2",
}


class ListDataSet:
    """In-memory stand-in for the reference's data sets: item = (systems_tril, solutions, right_hand_sides,
    original_sizes) with batch size 1, as `SludgePatternDataSet.__getitem__` returns (data_set.py:73-130)."""

    def __init__(self, matrices, right_hand_sides, solutions=None, dof_max: int | None = None, device="cuda"):
        self.matrices, self.rhs = list(matrices), list(right_hand_sides)
        self.solutions = list(solutions) if solutions is not None else [np.ones(m.shape[0]) for m in self.matrices]
        self.dof_max = max(m.shape[0] for m in self.matrices) if dof_max is None else dof_max
        self.device = device

    def __len__(self) -> int:
        return len(self.matrices)

    def __getitem__(self, index: int):
        m = self.matrices[index]
        tril, sizes = tril_batch_from_csr([m], dof_max=self.dof_max, device=self.device)
        pad = self.dof_max - m.shape[0]
        to = lambda v: torch.from_numpy(np.pad(np.asarray(v, dtype=np.float64), (0, pad), constant_values=1)).float().unsqueeze(0).to(self.device)  # noqa: E731
        return tril, to(self.solutions[index]), to(self.rhs[index]), sizes


@dataclass
class BenchmarkSuite:
    data_set: object
    model: torch.nn.Module | None
    techniques: tuple[str, ...] = ("vanilla", "jacobi", "incomplete_cholesky", "incomplete_cholesky_solve", "learned")
    results_directory: pathlib.Path = pathlib.Path("./assets/results/")
    kappa_max_n: int = 3000   # cond(M A) needs dense N x N matrices (test.py:111-113): beyond, a Lanczos estimate of the spectrum
    results: dict = field(default_factory=dict)

    def __post_init__(self):
        for p in PARAMETERS:
            setattr(self, p, {name: [] for name in self.techniques})
        # per technique and sample where its kappa came from: "dense" (cond of the dense M A, test.py:111-113), "lanczos"
        # (lambda_max / lambda_min of M A, device estimate beyond kappa_max_n) or "unconverged" (kappa is NaN)
        self.kappa_sources = {name: [] for name in self.techniques}

    # -- test.py:61-68 without densifying: mirror the strict lower triangle, compress on the device ----------
    def _reconstruct_system(self, system_tril, original_size: int) -> CsrSystem:
        assert system_tril.batch_size == 1, "Set batch size to one for testing"
        idx = system_tril.indices.long()
        keep = (idx[:, 1] < original_size) & (idx[:, 2] < original_size)
        r, c, v = idx[keep, 1], idx[keep, 2], system_tril.features[keep, 0].to(torch.float64)
        off = r != c
        rows = torch.cat((r, c[off]))
        cols = torch.cat((c, r[off]))
        vals = torch.cat((v, v[off]))
        rowptr, col, val = coo_to_csr_device(rows, cols, vals, original_size, device=v.device)
        return CsrSystem(rowptr, col, val, original_size)

    def _construct(self, name: str, system: CsrSystem, system_tril, original_size: int):
        if name == "vanilla":                       # test.py:70-72
            return Identity()
        if name == "jacobi":                        # test.py:74-79
            return Jacobi()
        if name == "incomplete_cholesky":           # test.py:81-88: icholt(add_fill_in=1, threshold=0.1) by default, and
            return ICholT("multiply", add_fill_in=1, threshold=0.1)   # the factor is MULTIPLIED, as the reference does
        if name == "incomplete_cholesky_level1":    # the static-pattern ICT of rounds 2-3 (opt-in)
            return ICT("multiply", fill_in=1, threshold=0.1)
        if name == "incomplete_cholesky_0":         # the reference's other branch (both arguments zeroed): ichol0
            return IC0("multiply")
        if name == "incomplete_cholesky_solve":     # IC(0) applied by triangular solves (not in the reference)
            return IC0("solve")
        if name == "incomplete_cholesky_multicolor":    # ... in multicolour order (opt-in: not among the default techniques)
            return IC0("solve", ordering="multicolor")
        if name == "incomplete_lu":                 # test.py:90-93 (opt-in): ilupp.ilut, the factors MULTIPLIED (M = L U)
            return ILUT("multiply", add_fill_in=1, threshold=0.1)
        if name == "sparse_approximate_inverse":    # FSAI on tril(A) (opt-in; not in the reference)
            return FSAI(level=1)
        if name == "sparse_approximate_inverse_level2":    # ... on the lower triangle of the pattern of A^2 (opt-in)
            return FSAI(level=2)
        if name == "algebraic_multigrid":           # test.py:95-98 (opt-in): smoothed aggregation, one V-cycle per update
            return SmoothedAggregation()
        if name == "algebraic_multigrid_gauss_seidel":     # the same hierarchy, multicolour Gauss-Seidel smoothing (opt-in)
            return SmoothedAggregation(smoother="gauss_seidel")
        if name == "algebraic_multigrid_chebyshev":        # the same hierarchy, Chebyshev smoothing (opt-in)
            return SmoothedAggregation(smoother="chebyshev")
        if name == "algebraic_multigrid_fp32":             # the same hierarchy, the cycle stored in fp32 (opt-in)
            return SmoothedAggregation(precision="fp32")
        if name == "learned":                       # test.py:100-105
            with torch.no_grad():
                out = self.model(system_tril)
            return LLtMultiply(lower_factor_csr(out, 0, original_size))
        raise ValueError(name)

    def _density_and_kappa(self, system: CsrSystem, n: int, want_spectrum: bool = False):
        """100 * nnz(M) / n^2 (test.py:107-109), cond(M A) (test.py:111-113) and, for the first sample, the singular
        values of M A (test.py:115-117) -- reporting only, dense N x N, small n only -- and where the kappa came from.
        Beyond kappa_max_n: kappa = lambda_max / lambda_min of M A by the device Lanczos estimator (CsrSystem.spectrum_bounds;
        the same number as the dense cond() only when M = c I), NaN when it did not converge; the density stays NaN."""
        if n > self.kappa_max_n:
            try:
                sb = system.spectrum_bounds(rtol=1e-4, max_steps=min(n, 2000))
            # M found not positive definite -- or, for incomplete_lu, M = L U not symmetric (dpcg_spectrum refuses it up front): no
            # number (as the dense path would give for an indefinite M A)
            except DpcgError as exc:
                if exc.status != BREAKDOWN:
                    raise
                return float("nan"), float("nan"), None, "unconverged"
            if sb.converged:
                return float("nan"), sb.kappa, None, "lanczos"
            return float("nan"), float("nan"), None, "unconverged"
        eye = torch.eye(n, dtype=torch.float64, device=system.device)
        M = torch.stack([system.precond_apply(eye[:, j]) for j in range(n)], dim=1)
        A = torch.stack([system @ eye[:, j] for j in range(n)], dim=1)
        density = 100.0 * float((M != 0).sum()) / (n * n)
        MA = M @ A
        spectrum = torch.linalg.svdvals(MA).tolist() if want_spectrum else None
        return density, float(torch.linalg.cond(MA)), spectrum, "dense"

    def run(self) -> None:
        """test.py:119-155."""
        for index in range(len(self.data_set)):
            system_tril, _, right_hand_side, original_size = self.data_set[index]
            n = int(original_size[0])
            system = self._reconstruct_system(system_tril, n)
            rhs = right_hand_side[0, :n].squeeze().to(torch.float64)
            eigenvalues = {}
            for name in self.techniques:
                torch.cuda.synchronize()
                start = time.perf_counter()
                system.set_preconditioner(self._construct(name, system, system_tril, n))
                torch.cuda.synchronize()
                setup = time.perf_counter() - start if name != "vanilla" else 0.0      # test.py:135
                duration, iteration, info = preconditioned_conjugate_gradient(system, rhs, system._precond)
                density, kappa, spectrum, source = self._density_and_kappa(system, n, want_spectrum=index == 0)
                self.kappa_sources[name].append(source)
                if spectrum is not None:
                    eigenvalues[name] = spectrum
                self._record(name, kappas=kappa, densities=density, iterations=iteration, setups=setup, durations=duration,
                             totals=setup + duration, successes=100 * (1 - info))      # the columns of test.py:143-149
            if index == 0 and eigenvalues:                                              # test.py:151-155
                self.results_directory.mkdir(parents=True, exist_ok=True)
                with (self.results_directory / "eigenvalues.csv").open(mode="w") as f:
                    f.write(",".join(eigenvalues.keys()) + "\n")
                    for row in zip(*eigenvalues.values()):
                        f.write(",".join(str(v) for v in row) + "\n")
            system.close()

    def _record(self, technique: str, **columns) -> None:
        """One sample's numbers of one technique into the per-technique lists (`self.kappas[technique]`, ...)."""
        assert set(columns) == set(PARAMETERS), sorted(columns)
        for parameter, value in columns.items():
            getattr(self, parameter)[technique].append(value)

    def dump_csv(self) -> None:
        """The files of test.py:175-198, same names, headers and cell formatting (`str` of a float): `table.csv` = one row per
        technique with the mean of every column of PARAMETERS, `totals.csv` = one row per sample with every technique's total."""
        import csv
        self.results_directory.mkdir(parents=True, exist_ok=True)

        def write(name, header, rows):
            with (self.results_directory / name).open(mode="w", newline="") as f:
                out = csv.writer(f, lineterminator="\n")
                out.writerow(header)
                out.writerows(rows)

        means = {t: [float(np.mean(getattr(self, col)[t], dtype=float)) for col in PARAMETERS] for t in self.techniques}
        write("table.csv", ["technique", *PARAMETERS], ([t, *means[t]] for t in self.techniques))
        write("comparability.csv", ["technique", "comparable_with_the_reference"],                # not in the reference: see COMPARABILITY
              ([t, COMPARABILITY.get(t, "unknown technique")] for t in self.techniques))
        write("totals.csv", self.techniques, zip(*(self.totals[t] for t in self.techniques)))
        if any(src == "lanczos" for srcs in self.kappa_sources.values() for src in srcs):   # not in the reference: see _density_and_kappa
            write("kappa_sources.csv", self.techniques, zip(*(self.kappa_sources[t] for t in self.techniques)))


def main(params_path="params.yaml", checkpoint="./assets/checkpoints/best.pt", root=None, *,
         allow_random_weights: bool = False) -> BenchmarkSuite:
    """test.py:201-221 without DVC: read `params.yaml` (keys `data`, `model`, `channels`), build the test split with
    batch size 1, load the checkpoint, run and dump the CSVs.  A missing checkpoint raises, as the reference's
    `torch.load` does (test.py:213) -- "learned" numbers from random weights would look plausible and mean nothing;
    `allow_random_weights=True` (tests, smoke runs without a trained model) opts into seeded random weights."""
    import yaml

    from . import data_set as data_sets
    from . import model as models
    assert torch.cuda.is_available(), "CUDA not available"                           # test.py:203
    torch.manual_seed(69)                                                            # test.py:205
    params = yaml.safe_load(pathlib.Path(params_path).read_text())
    kwargs = {} if root is None else {"root": pathlib.Path(root)}
    data = getattr(data_sets, params["data"])(stage="test", batch_size=1, shuffle=False, **kwargs)
    model = getattr(models, params["model"])(params["channels"])
    if pathlib.Path(checkpoint).exists():
        models.load_reference_state_dict(model, torch.load(checkpoint, map_location="cpu"))
    elif not allow_random_weights:
        raise FileNotFoundError(f"checkpoint {checkpoint} not found (pass allow_random_weights=True to benchmark a "
                                "randomly initialised model)")
    model = model.to("cuda")
    suite = BenchmarkSuite(data, model)
    suite.run()
    suite.dump_csv()
    return suite


if __name__ == "__main__":
    main()
