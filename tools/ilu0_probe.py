"""ILU(0) / DILU (D.ILU0, dpcg_ilu0.hip) under BiCGStab against Jacobi and ILUT on the systems of profiles/bicgstab_probe.md.

    python tools/ilu0_probe.py [OUT.md]   # on the GPU: writes profiles/ilu0_probe.md (or OUT.md)

`convection_diffusion_csr` at 64^3, 100^3 and 1024^2 (cell Peclet number 3), b = poisson.rhs(seed 0), rtol_sq = 1e-8, solved by
`solve_bicgstab` with Jacobi, ILU0 multicolour, ILU0 in the caller's order, ILU0(variant="dilu") multicolour and
ILUT("solve", threshold=1e-3).  ROUNDS rounds; in a round every preconditioner is attached in turn (setup ms: a host clock around the
attach, which ends in a device synchronise), warmed up by a 4-update call, and solved once (ms: the library's device-synchronised timer
of the loop).  The table holds the MEDIANS over the rounds and the spread (max - min) / median of ms to the solution; the
preconditioners alternate inside a round, so a drift of the machine touches them alike.  Everything in one process, on one commit.
"""

import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PROFILE = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "ilu0_probe.md"

SHAPES = [(64, 64, 64), (100, 100, 100), (1024, 1024)]
PECLET = 3.0
RTOL_SQ = 1e-8
MAX_ITER = 5000
ROUNDS = 5


def preconditioners(D):
    return [("Jacobi", lambda: D.Jacobi()),
            ('ILU0("solve", ordering="multicolor")', lambda: D.ILU0("solve", ordering="multicolor")),
            ('ILU0("solve", ordering="caller")', lambda: D.ILU0("solve", ordering="caller")),
            ('ILU0("solve", ordering="multicolor", variant="dilu")', lambda: D.ILU0("solve", ordering="multicolor", variant="dilu")),
            ('ILUT("solve", threshold=0.001)', lambda: D.ILUT("solve", threshold=1e-3))]


def main():
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson

    assert torch.cuda.is_available(), "this probe needs the GPU"
    name = torch.cuda.get_device_properties(0).gcnArchName
    lines = ["# ILU(0) and DILU under BiCGStab (dpcg_set_precond_ilu0)", "",
             f"`python tools/ilu0_probe.py` on {name}: convection-diffusion (first-order upwind, cell Peclet number {PECLET:g}), "
             f"b = poisson.rhs(seed 0), rtol_sq = {RTOL_SQ:g}; medians of {ROUNDS} rounds, the preconditioners alternating inside a round, each "
             "attach followed by a 4-update warm-up call and one timed solve.  spread: (max - min) / median of ms to the solution.  ms and "
             "us / update include the SpMVs of the updates the host had enqueued beyond the stop (see profiles/bicgstab_probe.md): that "
             "weighs on the solves of few updates.  vs Jacobi: ms to the solution over Jacobi's on the same system.", "",
             "| shape | rows | M | updates | us / update | ms to the solution | spread | vs Jacobi | setup ms | colours | levels L / U |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for shape in SHAPES:
        A = poisson.convection_diffusion_csr(shape, PECLET)
        rows = A.shape[0]
        b = poisson.rhs(rows, 0)
        S = D.CsrSystem.from_any(A)
        pcs = preconditioners(D)
        rec = {label: {"ms": [], "us": [], "setup": [], "updates": set(), "status": set()} for label, _ in pcs}
        for _ in range(ROUNDS):
            for label, make in pcs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.set_preconditioner(make())
                torch.cuda.synchronize()
                setup = (time.perf_counter() - t0) * 1e3
                S.solve_bicgstab(b, rtol_sq=RTOL_SQ, max_iter=4)
                res = S.solve_bicgstab(b, rtol_sq=RTOL_SQ, max_iter=MAX_ITER)
                r = rec[label]
                r["ms"].append(res.seconds * 1e3)
                r["us"].append(res.seconds / max(res.iterations, 1) * 1e6)
                r["setup"].append(setup)
                r["updates"].add(res.iterations)
                r["status"].add(res.status)
                r["colours"] = S.precond_ordering()[0] if label != "Jacobi" else 0
                info = S.info()
                r["levels"] = (info["levels_lower"], info["levels_upper"])
                if res.status == 0 and "true" not in r:
                    e = b.cpu().numpy() - A @ res.x.cpu().numpy()
                    r["true"] = float(e @ e) / float((b @ b).item())
        jac = statistics.median(rec["Jacobi"]["ms"])
        for label, _ in pcs:
            r = rec[label]
            ms = statistics.median(r["ms"])
            spread = (max(r["ms"]) - min(r["ms"])) / ms
            updates = "/".join(str(u) for u in sorted(r["updates"]))
            status = "" if r["status"] == {0} else f" (status {sorted(r['status'])})"
            levels = "-" if label == "Jacobi" else f"{r['levels'][0]} / {r['levels'][1]}"
            row = (f"| {' x '.join(str(d) for d in shape)} | {rows} | {label} | {updates}{status} | {statistics.median(r['us']):.2f} | {ms:.3f} | "
                   f"{100 * spread:.1f} % | {ms / jac:.2f} | {statistics.median(r['setup']):.3f} | {r['colours'] if label != 'Jacobi' else '-'} | {levels} |")
            print(row, f"(true residual {r.get('true', np.nan):.3e})", flush=True)
            lines.append(row)
        del S
    PROFILE.write_text("\n".join(lines) + "\n")
    print(f"wrote {PROFILE}")


if __name__ == "__main__":
    main()
