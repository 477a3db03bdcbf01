"""SmoothedAggregation's smoothers (dpcg_set_precond_amg_smoothed): Jacobi nu=1, multicolour Gauss-Seidel nu=1 and Chebyshev of
degree 2 and 3 on the systems of profiles/amg_probe.md -- setup, colours, launches, cycle cost, time to solution.

    python tools/amg_smoother_probe.py [--systems p3_100,...] --out profiles/amg_smoother_probe.jsonl
    DPCG_AMG_GS_BLOCK_ROWS=R python tools/amg_smoother_probe.py --gs-only --tag block_R --systems ... --out block.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sm -- \
        python tools/amg_smoother_probe.py --trace-only --systems p3_100 --out /dev/null
    python tools/amg_smoother_probe.py --render profiles/amg_smoother_probe.jsonl [block.jsonl ...] [--stats OUT/sm_kernel_stats.csv]

Per system and smoother: setup ms cold and re-attached after update_values (same pattern, new values), the smoother each level
uses and its colours (a Gauss-Seidel level that could not be coloured reports jacobi), launches of one cycle (the library's own
count, info()["precond_launches"] when present, else the formula of DESIGN.md), us per apply (HIP events around 50 applies),
iterations, us per PCG update and ms to solution (rtol_sq = 1e-8, max_iter = 1024, the wall time of a second solve).
--trace-only runs 50 applies of Gauss-Seidel and of Chebyshev (degree 2) per system and nothing else.
"""

import argparse
import csv
import json
import sys
import time

_ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path[:0] = [_ROOT, _ROOT + "/tools"]
from amg_probe import _systems, _time_applies  # noqa: E402

CONFIGS = [("jacobi_nu1", dict(smoother="jacobi")), ("gauss_seidel_nu1", dict(smoother="gauss_seidel")),
           ("chebyshev_k2", dict(smoother="chebyshev", degree=2)), ("chebyshev_k3", dict(smoother="chebyshev", degree=3))]


def _launches(info, kw):
    """Kernel launches of one V(1, 1) cycle (amg_launches in dpcg_amg.hip)."""
    import os
    block = int(os.environ.get("DPCG_AMG_GS_BLOCK_ROWS", "4096"))
    t = 1
    for l in range(info.levels - 1):
        if info.smoother[l] == "gauss_seidel":
            t += 5 if info.rows[l] <= block else 2 * (2 * info.colors[l] - 1) + 3
        elif info.smoother[l] == "chebyshev":
            t += 2 * kw.get("degree", 2) + 3
        else:
            t += 4
    return t


def _solve(S, b, precond):
    import torch
    S.set_preconditioner(precond)
    S.solve(b, rtol_sq=1e-8, max_iter=1024)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.solve(b, rtol_sq=1e-8, max_iter=1024)
    wall = time.perf_counter() - t0
    return {"iterations": res.iterations, "converged": res.status == 0, "ms_to_solution": round(1e3 * wall, 3),
            "us_per_update": round(1e6 * res.seconds / max(1, res.iterations), 2)}


def _handle(A):
    import torch
    import deeppreconditioning_amd as D
    if isinstance(A, tuple):
        rp, ci, v = A
        return D.CsrSystem(rp, ci, v, rp.numel() - 1), v
    return D.CsrSystem.from_any(A), torch.from_numpy(A.data).cuda()


def probe(name, A, configs, trace_only=False):
    import torch
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson
    S, vals = _handle(A)
    n = S.n
    b = poisson.rhs(n, 0, device="cuda")
    row = {"system": name, "rows": n, "nnz": S.info()["nnz"], "reordered": S.reordered}
    for key, kw in configs:
        pc = D.SmoothedAggregation(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(pc)
        cold = time.perf_counter() - t0
        if trace_only:
            _time_applies(S, n)
            continue
        S.update_values(vals)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(pc)
        warm = time.perf_counter() - t0
        info = S.amg_hierarchy()
        row[key] = {"setup_ms_cold": round(1e3 * cold, 2), "setup_ms_reattach": round(1e3 * warm, 2), "levels": info.levels,
                    "level_rows": info.rows, "smoother": info.smoother, "colors": info.colors,
                    "fallbacks": sum(1 for s in info.smoother if s != kw["smoother"]),
                    "launches_per_apply": _launches(info, kw), "us_per_apply": round(_time_applies(S, n), 2)}
        row[key].update(_solve(S, b, pc))
    S.close()
    return row


def render(paths, stats=None):
    rows = [json.loads(line) for p in paths for line in open(p) if line.strip()]
    print("| system | smoother | setup ms cold / re-attach | colours per level (fallbacks) | launches | us / apply | its | us / update "
          "| ms to solution |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        name = r["system"] + (" (reordered)" if r.get("reordered") else "") + (f" [{r['tag']}]" if r.get("tag") else "")
        for key, _ in CONFIGS:
            if key not in r:
                continue
            c = r[key]
            cols = "/".join(str(x) for x in c["colors"]) if key.startswith("gauss") else "-"
            fb = f" ({c['fallbacks']})" if c["fallbacks"] else ""
            its = f"{c['iterations']}" + ("" if c["converged"] else " (not conv.)")
            print(f"| {name} | {key} | {c['setup_ms_cold']} / {c['setup_ms_reattach']} | {cols}{fb} | {c['launches_per_apply']} | "
                  f"{c['us_per_apply']} | {its} | {c['us_per_update']} | {c['ms_to_solution']} |")
    if stats:
        print()
        print("| kernel | calls | total us | average us |")
        print("|---|---|---|---|")
        with open(stats) as f:
            for k in csv.DictReader(f):
                if "k_amg" in k["Name"]:
                    name = k["Name"].replace("(anonymous namespace)::", "").replace("dpcg::", "").replace("void ", "")
                    print(f"| `{name.split('(')[0][:70]}` | {k['Calls']} | {float(k['TotalDurationNs']) / 1e3:.1f} | "
                          f"{float(k['AverageNs']) / 1e3:.1f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="p3_100,p3_256,p2_1024,unstructured_3_100,quadtree_foam,quadtree_random,delaunay")
    ap.add_argument("--out")
    ap.add_argument("--tag", default="")
    ap.add_argument("--gs-only", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--render", nargs="+")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.render:
        render(a.render, a.stats)
        return
    configs = [c for c in CONFIGS if c[0] == "gauss_seidel_nu1"] if a.gs_only else CONFIGS
    if a.trace_only:
        configs = [CONFIGS[1], CONFIGS[2]]
    out = open(a.out, "w") if a.out else sys.stdout
    for name, A in _systems(a.systems.split(",")):
        row = probe(name, A, configs, a.trace_only)
        if a.tag:
            row["tag"] = a.tag
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(name, "done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
