"""dpcg_spectrum (CsrSystem.spectrum_bounds) timings and the reorthogonalisation kernels' bandwidth.

    python tools/spectrum_probe.py                    # whole estimates, 3-D Poisson + Jacobi at 22 K, 262 K, 1 M rows
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o lz -- python tools/spectrum_probe.py --steps 257
    python tools/spectrum_probe.py --report OUT/.../lz_kernel_trace.csv     # GB/s of k_lz_update at j = 64, 256 (1 M rows)

`--steps K` runs K steps (rtol = 0) at 1 M rows: the k-th launch of each k_lz_update form is step j = k, so a kernel trace
gives every step's duration at a known basis width.  Bytes per launch count the basis columns and the work vectors each form
streams (partials are < 1 %).
"""

import argparse
import csv
import json
import sys
import time

import numpy as np

HBM_CEILING_GBS = 6290.0   # measured float4-copy rate of an MI355X (MI355X_MICROARCH.md)


def _system(D, O, m):
    S = D.CsrSystem.from_any(O.poisson3d(m))
    S.set_preconditioner(D.Jacobi())
    return S


def run_estimates():
    import torch
    import deeppreconditioning_amd as D
    from oracle import oracle as O
    out = []
    for m in (28, 64, 100):
        S = _system(D, O, m)
        S.spectrum_bounds(max_steps=16, rtol=0.0)          # warm-up: code objects, block cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sb = S.spectrum_bounds()
        dt = time.perf_counter() - t0
        row = {"rows": S.n, "steps": sb.steps, "converged": sb.converged, "seconds": round(dt, 4),
               "ms_per_step": round(1e3 * dt / sb.steps, 4), "kappa": sb.kappa, "lambda_min": sb.lambda_min,
               "lambda_max": sb.lambda_max}
        print(json.dumps(row), flush=True)
        out.append(row)
        S.close()
    return out


def run_steps(k):
    import deeppreconditioning_amd as D
    from oracle import oracle as O
    S = _system(D, O, 100)
    sb = S.spectrum_bounds(max_steps=k, rtol=0.0)
    print(json.dumps({"rows": S.n, "steps": sb.steps}))


def report(trace_csv, n=100 ** 3, widths=(64, 256)):
    ld = (n + 1023) // 1024 * 1024
    launches = {0: [], 1: [], 2: []}
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for mode in (0, 1, 2):
                if f"k_lz_update<{mode}," in name:
                    launches[mode].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows = []
    for mode, lst in launches.items():
        lst.sort()
        for j in widths:
            if j >= len(lst):
                continue
            cols = j + 1
            vecs = {0: cols + 3 + (1 if j > 0 else 0), 1: 2 * cols + 2, 2: cols + 2}[mode]   # columns streamed + w read and written
            nbytes = 8 * ld * vecs
            ns = lst[j][1] - lst[j][0]
            gbs = nbytes / ns
            rows.append({"kernel": f"k_lz_update<{mode}>", "j": j, "us": round(ns / 1e3, 2), "GB": round(nbytes / 1e9, 3),
                         "GB/s": round(gbs, 1), "frac_of_6.29TB/s": round(gbs / HBM_CEILING_GBS, 3)})
    for r in rows:
        print(json.dumps(r))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--report", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ".")
    if a.report:
        report(a.report)
    elif a.steps:
        run_steps(a.steps)
    else:
        run_estimates()
