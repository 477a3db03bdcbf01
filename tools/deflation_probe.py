"""What deflated PCG (dpcg_deflation.hip) costs per update and whether it pays to the solution.

    python tools/deflation_probe.py            # writes profiles/deflation_probe.md

Systems: the 2-D Poisson matrix on 256 x 256 (65 536 rows) and the 3-D one on 100^3 (1 M rows), Jacobi, b = poisson.rhs(seed 0).
us per update: exactly UPDATES updates (rtol_sq = 0 never passes), the driver's own loop time, best of REPEATS after one warm-up,
the variants ALTERNATING inside every repetition: the default path (whatever dpcg_solve chooses), the multi-launch path as three
plain launches per update (DPCG_NO_SMALL | DPCG_NO_TEAM | DPCG_NO_FUSE | DPCG_NO_GRAPH: the form the deflated driver has), and the
deflated driver with k = 1, 4, 8 subdomain indicators.  The extra traffic of deflation is 16 k bytes per row and update (AW in K2d,
W in K3d); its achieved rate is those bytes over the time added to the three-launch path, set against the library's streaming
kernel (dpcg_stream_bench, triad shape).  Time to the solution (rtol_sq = 1e-8): the default solve against "ritz" k = 8 and 8
subdomain indicators, best of 3 each, the harvest (Lanczos + attach) timed separately, once.
"""

import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import deeppreconditioning_amd as D  # noqa: E402
from deeppreconditioning_amd import _lib as L  # noqa: E402
from deeppreconditioning_amd.operators import stream_bench  # noqa: E402
from deeppreconditioning_amd.poisson import poisson_system, rhs, subdomain_indicators  # noqa: E402

UPDATES, REPEATS = 300, 5
PLAIN3 = L.NO_SMALL | L.NO_TEAM | L.NO_FUSE | L.NO_GRAPH
SYSTEMS = [("256x256", 2, 256, {1: (1, 1), 4: (2, 2), 8: (2, 4)}), ("100x100x100", 3, 100, {1: (1, 1, 1), 4: (2, 2, 1), 8: (2, 2, 2)})]


def jacobi_system(dim, n):
    S = poisson_system(dim, n)
    S.set_preconditioner(D.Jacobi())
    return S


def one_run(S, b, flags):
    res = S.solve(b, rtol_sq=0.0, max_iter=UPDATES, flags=flags, want_history=False)
    assert res.iterations == UPDATES and res.status == L.MAX_ITER, (res.iterations, res.status)
    return res.seconds / UPDATES * 1e6


def verdict(new, old):
    r = new / old
    return "a win" if r < 0.97 else ("a loss" if r > 1.03 else "a draw")


def main():
    torch.cuda.set_device(0)
    name = torch.cuda.get_device_properties(0).gcnArchName
    triad = stream_bench(2, True, 1 << 28, 10)
    lines = ["# Deflated PCG: cost per update and time to the solution", "",
             f"`python tools/deflation_probe.py` on {name}.  Jacobi, b = poisson.rhs(seed 0).  Streaming kernel of the library (triad shape, "
             f"dpcg_stream_bench): {triad:.0f} GB/s.", ""]
    per_update, to_solution = [], []
    for label, dim, n, blocks in SYSTEMS:
        shape = (n,) * dim
        rows = n ** dim
        b = rhs(rows, 0)
        variants = {"default": (jacobi_system(dim, n), 0), "3 plain launches": (jacobi_system(dim, n), PLAIN3)}
        for k, blk in blocks.items():
            S = jacobi_system(dim, n)
            S.set_deflation(subdomain_indicators(shape, blk))
            variants[f"deflated k={k}"] = (S, 0)
        best = {v: np.inf for v in variants}
        for rep in range(REPEATS + 1):
            for v, (S, flags) in variants.items():                       # alternating
                t = one_run(S, b, flags)
                if rep > 0:
                    best[v] = min(best[v], t)
        print(label, best, flush=True)
        per_update.append((label, rows, best))
        del variants
        # time to the solution
        S = jacobi_system(dim, n)
        sol = {}

        def timed(tag):
            runs = [S.solve(b, rtol_sq=1e-8, max_iter=20000, want_history=False) for _ in range(4)][1:]
            assert all(r.status == L.OK for r in runs), tag
            sol[tag] = (min(r.seconds for r in runs) * 1e3, runs[0].iterations)

        timed("default")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_deflation("ritz", k=8, max_steps=200, rtol=1e-3)
        torch.cuda.synchronize()
        harvest_ms = (time.perf_counter() - t0) * 1e3
        info = S.deflation()
        harvest_steps, harvest_ok = info["steps"], info["converged"]
        del info
        timed("ritz k=8")
        t0 = time.perf_counter()
        S.set_deflation(subdomain_indicators(shape, blocks[8]))
        torch.cuda.synchronize()
        attach_ms = (time.perf_counter() - t0) * 1e3
        timed("8 subdomain indicators")
        print(label, sol, harvest_ms, harvest_steps, harvest_ok, attach_ms, flush=True)
        to_solution.append((label, rows, sol, harvest_ms, harvest_steps, harvest_ok, attach_ms))
        del S
        L.lib().dpcg_release_cached_memory()

    cols = ["default", "3 plain launches", "deflated k=1", "deflated k=4", "deflated k=8"]
    lines += ["## us per update", "", f"{UPDATES} updates per run, best of {REPEATS} after a warm-up, variants alternating inside every repetition.", "",
              "| system | rows | " + " | ".join(cols) + " |", "|---|---|" + "---|" * len(cols)]
    for label, rows, best in per_update:
        lines.append(f"| {label} | {rows} | " + " | ".join(f"{best[c]:.2f}" for c in cols) + " |")
    lines += ["", "## The extra bytes", "", "16 k bytes per row and update over the time added to the three-launch path.", "",
              "| system | k | extra bytes per update | added us | achieved GB/s | of the streaming kernel |", "|---|---|---|---|---|---|"]
    for label, rows, best in per_update:
        for k in (1, 4, 8):
            extra = 16.0 * k * rows
            added = best[f"deflated k={k}"] - best["3 plain launches"]
            rate = extra / (added * 1e-6) / 1e9 if added > 0 else float("inf")
            lines.append(f"| {label} | {k} | {extra / 1e6:.2f} MB | {added:.2f} | {rate:.0f} | {100 * rate / triad:.0f} % |")
    lines += ["", "## Time to the solution (rtol_sq = 1e-8)", "", "Loop time of dpcg_solve, best of 3 after a warm-up; the harvest and the attach are one-off costs, timed once "
              "(host wall clock, device-synchronised).", "",
              "| system | variant | updates | ms | against default | one-off ms |", "|---|---|---|---|---|---|"]
    for label, rows, sol, harvest_ms, steps, ok, attach_ms in to_solution:
        d_ms = sol["default"][0]
        lines.append(f"| {label} | default | {sol['default'][1]} | {d_ms:.3f} | | |")
        ms, it = sol["ritz k=8"]
        lines.append(f"| {label} | ritz k=8 ({steps} Lanczos steps{'' if ok else ', not converged'}) | {it} | {ms:.3f} | {verdict(ms, d_ms)} ({ms / d_ms:.2f}x) | {harvest_ms:.1f} |")
        ms, it = sol["8 subdomain indicators"]
        lines.append(f"| {label} | 8 subdomain indicators | {it} | {ms:.3f} | {verdict(ms, d_ms)} ({ms / d_ms:.2f}x) | {attach_ms:.1f} |")
    path = ROOT / "profiles" / "deflation_probe.md"
    path.parent.mkdir(exist_ok=True)
    path.write_text("\n".join(lines) + "\n")
    print(path.read_text())


if __name__ == "__main__":
    main()
