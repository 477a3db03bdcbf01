"""SmoothedAggregation (dpcg_set_precond_amg) against Jacobi and multicolour IC(0): setup, V-cycle cost, time to solution.

    python tools/amg_probe.py [--systems p3_100,p3_256,...] [--sweeps 1,2] --out profiles/amg_probe.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o amg -- \
        python tools/amg_probe.py --trace-only --systems p3_100,quadtree_foam,delaunay --out levels.jsonl
    python tools/amg_probe.py --report OUT/amg_kernel_trace.csv levels.jsonl --ceiling GBS > profiles/amg_level0_kernels.jsonl
    python tools/amg_probe.py --render profiles/amg_probe.jsonl profiles/amg_level0_kernels.jsonl     # the tables of profiles/amg_probe.md

Per system: setup ms cold and re-attached after update_values (same pattern, new values), levels, rows per level, operator and
grid complexity, launches of one cycle, us per apply (HIP events around 50 applies), us per PCG update and iterations / ms to
solution (rtol_sq = 1e-8, max_iter = 1024, the reference's defaults) for AMG, Jacobi and IC(0) in multicolour order, and the
V-cycle's bytes / time against the measured streaming ceiling (D.stream_bench, a triad).  Bytes per cycle count, per level
and kernel, the matrix streams (12 B per entry + 4 B per row pointer) and the vectors each kernel reads and writes once.
--trace-only runs 50 applies per system and nothing else (a kernel trace of the cycle's kernels).
"""

import argparse
import csv
import json
import sys
import time

import numpy as np


def _systems(names):
    from deeppreconditioning_amd import meshes, poisson
    from oracle import oracle as O
    make = {
        "p3_100": lambda: poisson.poisson_csr(3, 100),
        "p3_256": lambda: poisson.poisson_csr(3, 256),
        "p2_1024": lambda: poisson.poisson_csr(2, 1024),
        "unstructured_3_100": lambda: poisson.unstructured_like_csr(3, 100),
        "quadtree_foam": lambda: meshes.quadtree_fv_laplacian(1000, 0),
        "quadtree_random": lambda: meshes.quadtree_fv_laplacian(1000, 0, numbering="random"),
        "delaunay": lambda: meshes.delaunay_laplacian(1000000, 0),
    }
    for name in names:
        yield name, make[name]()
    del O


def _cycle_bytes(info, sweeps):
    """Matrix and vector bytes one V(sweeps, sweeps) cycle moves (each kernel reads its matrix once)."""
    total = 0.0
    for l in range(info.levels - 1):
        n, nnz, pn, nc = info.rows[l], info.nnz[l], info.p_nnz[l], info.rows[l + 1]
        mat = 12.0 * nnz + 4.0 * (n + 1)
        pmat = 12.0 * pn + 4.0 * (n + 1)
        ptmat = 12.0 * pn + 4.0 * (nc + 1)
        total += sweeps * (mat + 8.0 * 4 * n)          # PRE/SWEEP: b (or x, r), dinv gathered; x, r written
        total += sweeps * (mat + 8.0 * 4 * n)          # POST: x, b, dinv; x written
        total += ptmat + 8.0 * (n + nc)                # restriction
        total += pmat + 8.0 * (2 * n + nc)             # prolongation with correction
    nco = info.rows[-1]
    total += 8.0 * nco * nco + 16.0 * nco
    return total


def _time_applies(S, n, reps=50):
    import torch
    r = torch.rand(n, device="cuda", dtype=torch.float64)
    S.precond_apply(r)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        S.precond_apply(r)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def _solve(S, b, precond):
    import torch
    S.set_preconditioner(precond)
    S.solve(b, rtol_sq=1e-8, max_iter=1024)           # warm-up (graph capture, code objects)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.solve(b, rtol_sq=1e-8, max_iter=1024)
    wall = time.perf_counter() - t0
    return {"iterations": res.iterations, "converged": res.status == 0, "final_res": res.final_res,
            "ms_to_solution": round(1e3 * wall, 3), "us_per_update": round(1e6 * res.seconds / max(1, res.iterations), 2)}


def probe(name, A, sweeps_list, ceiling):
    import torch
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson
    if isinstance(A, tuple):
        rp, ci, v = A
        S = D.CsrSystem(rp, ci, v, rp.numel() - 1)
        vals = v
    else:
        S = D.CsrSystem.from_any(A)
        vals = torch.from_numpy(A.data).cuda()
    n = S.n
    b = poisson.rhs(n, 0, device="cuda")
    row = {"system": name, "rows": n, "nnz": S.info()["nnz"], "reordered": S.reordered}
    for sweeps in sweeps_list:
        pc = D.SmoothedAggregation(sweeps=sweeps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(pc)
        cold = time.perf_counter() - t0
        S.update_values(vals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(pc)
        warm = time.perf_counter() - t0
        info = S.amg_hierarchy()
        us = _time_applies(S, n)
        nbytes = _cycle_bytes(info, sweeps)
        key = f"amg_nu{sweeps}"
        row[key] = {"setup_ms_cold": round(1e3 * cold, 2), "setup_ms_reattach": round(1e3 * warm, 2), "levels": info.levels,
                    "level_rows": info.rows, "rho": [round(x, 4) for x in info.rho],
                    "operator_complexity": round(info.operator_complexity, 3), "grid_complexity": round(info.grid_complexity, 3),
                    "launches_per_apply": (info.levels - 1) * (2 + 2 * sweeps) + 1, "us_per_apply": round(us, 2),
                    "cycle_mbytes": round(nbytes / 1e6, 1), "cycle_gbs": round(nbytes / (us * 1e3), 1),
                    "frac_of_stream_ceiling": round(nbytes / (us * 1e3) / ceiling, 3)}
        row[key].update(_solve(S, b, pc))
    row["jacobi"] = _solve(S, b, D.Jacobi())
    try:
        row["ic0_multicolor"] = _solve(S, b, D.IC0("solve", ordering="multicolor"))
    except D._lib.DpcgError as exc:
        row["ic0_multicolor"] = {"error": str(exc)}
    S.close()
    return row


def _level_sizes(S):
    info = S.amg_hierarchy()
    return {"levels": info.levels, "rows": info.rows, "nnz": info.nnz, "p_nnz": info.p_nnz}


def level0_report(trace_csv, levels_jsonl, ceiling):
    """Level-0 kernels of the cycle from a --trace-only kernel trace: median us, bytes, GB/s, fraction of the ceiling.

    Per apply (nu = 1) the cycle's kernels run in a fixed order -- PRE, PLAIN per level down, the GEMV, ACC, POST per level up --
    so level 0's PRE / restriction sit 2 (L - 1) and 2 (L - 1) - 1 launches before each GEMV, its prolongation / POST 2 (L - 1) - 1
    and 2 (L - 1) after it.  Each system ran 51 applies (one warm-up)."""
    systems = [json.loads(line) for line in open(levels_jsonl) if line.strip()]
    rows = []
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            if "k_amg_row" in r["Kernel_Name"] or "k_amg_gemv" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    gemv = [i for i, r in enumerate(rows) if "k_amg_gemv" in r[2]]
    out = []
    for si, sysinfo in enumerate(systems):
        L = sysinfo["levels"]
        n, nnz, pn, nc = sysinfo["rows"][0], sysinfo["nnz"][0], sysinfo["p_nnz"][0], sysinfo["rows"][1]
        h = 2 * (L - 1)
        kernels = {"pre (x = wD^-1 b, r = b - Ax)": (-h, "k_amg_row<0,", 12.0 * nnz + 4.0 * (n + 1) + 8.0 * 4 * n),
                   "restriction (b_1 = P^T r)": (-h + 1, "k_amg_row<4,", 12.0 * pn + 4.0 * (nc + 1) + 8.0 * (n + nc)),
                   "prolongation (x += P x_1)": (h - 1, "k_amg_row<3,", 12.0 * pn + 4.0 * (n + 1) + 8.0 * (2 * n + nc)),
                   "post (x += wD^-1 (b - Ax), <r, z>)": (h, "k_amg_row<2,", 12.0 * nnz + 4.0 * (n + 1) + 8.0 * 4 * n)}
        mine = gemv[si * 51 + 1:(si + 1) * 51]          # (the warm-up apply left out)
        for label, (off, prefix, nbytes) in kernels.items():
            durs = []
            for g in mine:
                name = rows[g + off][2]
                assert prefix in name.replace(" ", ""), (label, name)
                durs.append(rows[g + off][1])
            us = float(np.median(durs)) / 1e3
            gbs = nbytes / (us * 1e3)
            out.append({"system": sysinfo["system"], "kernel": label, "us": round(us, 2), "mbytes": round(nbytes / 1e6, 1),
                        "gbs": round(gbs, 1), "frac_of_ceiling": round(gbs / ceiling, 3)})
    return out


def render(probe_jsonl, kernels_jsonl=None):
    """profiles/amg_probe.md from the probe's JSONL (and the level-0 kernel rows of level0_report)."""
    lines = [json.loads(line) for line in open(probe_jsonl) if line.strip()]
    ceiling = next(r["stream_ceiling_gbs"] for r in lines if "stream_ceiling_gbs" in r)
    md = ["| system | rows | levels (rows) | op. / grid cx | setup ms cold / re-attach | launches | us / apply | AMG nu=1 its / us per update / ms | "
          "AMG nu=2 its / us per update / ms | Jacobi its / us per update / ms | IC(0) mc its / us per update / ms |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]

    def cell(d):
        if "error" in d:
            return "error"
        return f"{d['iterations']}{'' if d['converged'] else ' (not conv.)'} / {d['us_per_update']:.1f} / {d['ms_to_solution']:.2f}"
    for r in lines:
        if "system" not in r:
            continue
        if "error" in r:
            md.append(f"| {r['system']} | error: {r['error']} |")
            continue
        a = r["amg_nu1"]
        md.append(f"| {r['system']}{' (reordered)' if r['reordered'] else ''} | {r['rows']:,} | {a['levels']} "
                  f"({', '.join(str(x) for x in a['level_rows'])}) | {a['operator_complexity']:.2f} / {a['grid_complexity']:.2f} | "
                  f"{a['setup_ms_cold']:.1f} / {a['setup_ms_reattach']:.1f} | {a['launches_per_apply']} | {a['us_per_apply']:.0f} | "
                  f"{cell(a)} | {cell(r['amg_nu2'])} | {cell(r['jacobi'])} | {cell(r['ic0_multicolor'])} |")
    md.append(f"\nStreaming ceiling (`stream_bench`, triad walked by the whole grid): {ceiling:.0f} GB/s.")
    if kernels_jsonl:
        md += ["", "| system | level-0 kernel | us (median of 50) | MB | GB/s | of ceiling |", "|---|---|---|---|---|---|"]
        for k in (json.loads(line) for line in open(kernels_jsonl) if line.strip()):
            md.append(f"| {k['system']} | {k['kernel']} | {k['us']:.1f} | {k['mbytes']:.1f} | {k['gbs']:.0f} | {k['frac_of_ceiling']:.2f} |")
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="p3_100,p3_256,p2_1024,unstructured_3_100,quadtree_foam,quadtree_random,delaunay")
    ap.add_argument("--sweeps", default="1,2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--report", nargs=2, metavar=("KERNEL_TRACE_CSV", "LEVELS_JSONL"), help="level-0 kernels of a --trace-only trace")
    ap.add_argument("--ceiling", type=float, default=None, help="GB/s (--report)")
    ap.add_argument("--render", nargs="+", metavar="JSONL", help="markdown table from the probe's JSONL [and --report's]")
    args = ap.parse_args()
    if args.render:
        print(render(*args.render))
        return 0
    if args.report:
        for row in level0_report(args.report[0], args.report[1], args.ceiling):
            print(json.dumps(row))
        return 0
    import deeppreconditioning_amd as D
    names = args.systems.split(",")
    out = open(args.out, "w") if args.out else None
    if args.trace_only:
        for name, A in _systems(names):
            S = D.CsrSystem(*A, A[0].numel() - 1) if isinstance(A, tuple) else D.CsrSystem.from_any(A)
            S.set_preconditioner(D.SmoothedAggregation())
            _time_applies(S, S.n)
            line = json.dumps({"system": name, **_level_sizes(S)})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
            S.close()
        return 0
    ceiling = D.operators.stream_bench(n_read=2, write=True, out_bytes=1 << 28, repeats=10, walk=True)
    line = json.dumps({"stream_ceiling_gbs": round(ceiling, 1)})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
    for name, A in _systems(names):
        try:
            row = probe(name, A, [int(s) for s in args.sweeps.split(",")], ceiling)
        except Exception as exc:          # one system's failure is reported, the others still run
            row = {"system": name, "error": f"{type(exc).__name__}: {exc}"}
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
