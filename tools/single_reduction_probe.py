"""The single-reduction recurrence (DPCG_SINGLE_REDUCTION, dpcg_chip_sr.hip) beside the standard whole-chip kernel.

    python tools/single_reduction_probe.py --out profiles/single_reduction_probe.md

Per system (Poisson 41^3, 64^3, 80^3, 100^3 and 1024^2 with Jacobi, b ~ U(-1, 1), rtol_sq = 1e-8, at most 1024 updates): microseconds
per update of the kernel between HIP events on its stream (DPCG_CHIP_EVENTS=1, `chip_info()["kernel_ms"]` over the updates), updates
and milliseconds to the solution -- or, where the solve ends at the cap of 1024 updates unconverged, updates and milliseconds to the
cap ("capped" in the status column).  One process, the two recurrences alternating and swapping who goes first,
--passes passes (at least 7): median and least .. most.  A system the variant does not take is reported as refused, with the reason.
"""

import argparse
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/single_reduction_probe.md")
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    passes = max(7, args.passes)
    os.environ["DPCG_CHIP_EVENTS"] = "1"
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    import torch
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson

    lines = ["# Single-reduction recurrence against the standard whole-chip kernel", "",
             f"{torch.cuda.get_device_name(0)}; Jacobi, rtol_sq = 1e-8, max_iter = 1024; {passes} alternating passes in one process; "
             "median (least .. most).", "",
             "| system | rows | recurrence | status | updates | us per update | ms to the solution (capped: to the cap) |", "|---|---|---|---|---|---|---|"]
    verdicts = []
    for name, dim, m in (("41^3", 3, 41), ("64^3", 3, 64), ("80^3", 3, 80), ("100^3", 3, 100), ("1024^2", 2, 1024)):
        S = poisson.poisson_system(dim, m)
        S.set_preconditioner(D.Jacobi())
        n = S.n
        b = poisson.rhs(n, 0)
        stats = {"standard": [], "single_reduction": []}
        refused = None
        for p in range(passes + 1):                      # (pass 0 warms both up and is dropped)
            order = ("standard", "single_reduction") if p % 2 == 0 else ("single_reduction", "standard")
            for rec in order:
                if rec == "single_reduction" and refused:
                    continue
                try:
                    r = S.solve(b, recurrence=rec, want_history=False)
                except D._lib.DpcgError as e:
                    refused = str(e)
                    continue
                assert r.recurrence == rec, (name, rec, r.recurrence)
                ms = S.chip_info()["kernel_ms"]
                if p > 0:
                    stats[rec].append((r.iterations, 1e3 * ms / max(r.iterations, 1), ms, r.status))
        med = {}
        for rec in ("standard", "single_reduction"):
            if not stats[rec]:
                lines.append(f"| {name} | {n} | {rec} | refused: {refused} | | | |")
                continue
            its = sorted({s[0] for s in stats[rec]})
            us = [s[1] for s in stats[rec]]
            ms = [s[2] for s in stats[rec]]
            med[rec] = (statistics.median(us), min(us), max(us), statistics.median(ms), min(ms), max(ms))
            st = "/".join(sorted({("converged", "capped", "breakdown")[s[3]] for s in stats[rec]}))
            lines.append(f"| {name} | {n} | {rec} | {st} | {'/'.join(map(str, its))} | {statistics.median(us):.2f} ({min(us):.2f} .. {max(us):.2f}) | "
                         f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f}) |")
        if len(med) == 2:
            a, v = med["standard"], med["single_reduction"]
            apart = v[5] < a[4] or a[5] < v[4]           # the ranges of ms to the solution do not overlap
            what = "ms to the cap of 1024 updates" if any(s[3] == 1 for s in stats["standard"] + stats["single_reduction"]) else "ms to the solution"
            verdicts.append(f"* {name}: {what} {v[3] / a[3]:.3f} x the standard kernel's"
                            f" ({'separated beyond the spread' if apart else 'within the spread'}).")
        S.close()
    lines += ["", "Medians of the variant over the standard kernel:", ""] + verdicts
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
