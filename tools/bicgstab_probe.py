"""BiCGStab (CsrSystem.solve_bicgstab, dpcg_bicgstab.hip) on convection-diffusion systems: us per update and ms to the solution.

    python tools/bicgstab_probe.py [OUT.md]   # on the GPU: writes profiles/bicgstab_probe.md (or OUT.md)

`convection_diffusion_csr` at 64^3, 100^3 and 1024^2 (cell Peclet number 3), with Jacobi and ILUT("solve", threshold=1e-3) -- ILUT's
default threshold 0.1 keeps only the diagonal of these matrices; the probe prints what the factors keep --, each case ONCE after one
untimed warm-up call of 4 updates (allocations, the triangular schedules), at rtol_sq = 1e-8: updates, status, ms of the loop (the
library's device-synchronised timer) and us per update.  Beside them the us per update of `solve` with DPCG_NO_SMALL -- the multi-launch
PCG path, Jacobi -- on the SPD Poisson system of the same shape.  A BiCGStab update is two SpMVs and three vector passes where a PCG
update is one SpMV and two passes, so roughly twice that figure is the expectation to compare against.  It is not a bar.
"""

import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PROFILE = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "bicgstab_probe.md"

SHAPES = [(64, 64, 64), (100, 100, 100), (1024, 1024)]
PECLET = 3.0
RTOL_SQ = 1e-8
MAX_ITER = 5000
ILUT_THRESHOLD = 1e-3


def main():
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson

    assert torch.cuda.is_available(), "this probe needs the GPU"
    name = torch.cuda.get_device_properties(0).gcnArchName
    lines = ["# BiCGStab (dpcg_solve_bicgstab)", "", f"`python tools/bicgstab_probe.py` on {name}: convection-diffusion (first-order upwind, "
             f"cell Peclet number {PECLET:g}), b = poisson.rhs(seed 0), rtol_sq = {RTOL_SQ:g}, every case once after a 4-update warm-up.  "
             "PCG us / update: `solve(flags=NO_SMALL)` with Jacobi on the Poisson system of the same shape (the multi-launch path); about "
             "twice that is what two SpMVs and three passes should cost.  ms and us / update include the two SpMVs of each update the host had "
             "enqueued beyond the stop (up to 32 updates): they have no control word and run in full.", "",
             "| shape | rows | M | updates | status | ms to the solution | us / update | PCG us / update | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    for shape in SHAPES:
        A = poisson.convection_diffusion_csr(shape, PECLET)
        rows = A.shape[0]
        b = poisson.rhs(rows, 0)
        P = poisson.poisson_system(len(shape), shape[0])
        P.set_preconditioner(D.Jacobi())
        P.solve(b, rtol_sq=RTOL_SQ, max_iter=4, flags=D._lib.NO_SMALL)
        pcg = P.solve(b, rtol_sq=RTOL_SQ, max_iter=MAX_ITER, flags=D._lib.NO_SMALL, want_history=False)
        pcg_us = pcg.seconds / max(pcg.iterations, 1) * 1e6
        del P
        S = D.CsrSystem.from_any(A)
        for label, M in (("Jacobi", D.Jacobi()), (f'ILUT("solve", threshold={ILUT_THRESHOLD:g})', D.ILUT("solve", threshold=ILUT_THRESHOLD))):
            S.set_preconditioner(M)
            if label != "Jacobi":
                Lf, Uf = S.lu_factors()
                label += f": {Lf.nnz - rows} + {Uf.nnz - rows} off-diagonal entries"
            S.solve_bicgstab(b, rtol_sq=RTOL_SQ, max_iter=4)
            res = S.solve_bicgstab(b, rtol_sq=RTOL_SQ, max_iter=MAX_ITER)
            us = res.seconds / max(res.iterations, 1) * 1e6
            true = np.nan
            if res.status == 0:
                e = b.cpu().numpy() - A @ res.x.cpu().numpy()
                true = float(e @ e) / float((b @ b).item())
            row = (f"| {' x '.join(str(d) for d in shape)} | {rows} | {label} | {res.iterations} | {res.status} | {res.seconds * 1e3:.3f} | {us:.2f} | "
                   f"{pcg_us:.2f} | {us / pcg_us:.2f} |")
            print(row, f"(true residual {true:.3e})", flush=True)
            lines.append(row)
        del S
    PROFILE.write_text("\n".join(lines) + "\n")
    print(f"wrote {PROFILE}")


if __name__ == "__main__":
    main()
