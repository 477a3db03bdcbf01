"""Block-Jacobi incomplete Cholesky (D.BlockIC) against Jacobi and the global IC(0) solves: cost of an apply, of a PCG update, and
time to solution.

    python tools/block_ic_probe.py --out profiles/block_ic_probe.jsonl
    python tools/block_ic_probe.py --render profiles/block_ic_probe.jsonl        # the tables of profiles/block_ic_probe.md

Per system one handle per preconditioner, all alive in one process; every figure is the median of --passes (>= 5) passes that
alternate over the preconditioners, with the spread (min .. max) beside it.  us per apply: 20 dpcg_precond_apply calls between two
synchronisations.  us per update and ms to solution: dpcg_solve to rtol_sq = 1e-8 (its own timer over the updates; the wall time of
the call).  Blocks: boxes of about 512, 1000 and 4096 rows (grids: poisson.subdomain_blocks; the quadtree mesh has no boxes: runs of
its own numbering) and contiguous runs of 1024 rows -- in the natural order of a 2-D grid a run is a few grid lines, a long chain:
the level counts say so.  Apply bytes: what the solve kernel must move at least (per off-diagonal entry a value and a 16-bit column
for L and for L^T, per row two diagonals, two 16-bit row indices, two entry offsets, r twice and z through a 4-byte map) over the
measured time, beside the library's streaming kernel (dpcg_stream_bench) on the same device.
"""

import argparse
import json
import statistics
import sys
import time


def _systems(names):
    from deeppreconditioning_amd import meshes
    from deeppreconditioning_amd.poisson import subdomain_blocks as boxes
    from oracle import oracle as O
    make = {
        "poisson2d_256": lambda: (O.poisson2d(256), {"boxes~512": boxes((256, 256), (11, 11)), "boxes~1000": boxes((256, 256), (8, 8)),
                                                      "boxes~4096": boxes((256, 256), (4, 4)), "runs of 1024": 1024}),
        "poisson3d_100": lambda: (O.poisson3d(100), {"boxes~512": boxes((100,) * 3, (13,) * 3), "boxes~1000": boxes((100,) * 3, (10,) * 3),
                                                      "boxes~4096": boxes((100,) * 3, (7,) * 3), "runs of 1024": 1024}),
        "quadtree_1m": lambda: (meshes.quadtree_fv_laplacian(1000, 5), {"runs of 512": 512, "runs of 1000": 1000, "runs of 4096": 4096,
                                                                        "runs of 1024": 1024}),
        "poisson2d_48": lambda: (O.poisson2d(48), {"boxes~256": boxes((48, 48), (3, 3)), "runs of 1024": 1024}),      # (a quick self-test)
    }
    for name in names:
        yield (name,) + make[name]()


def _med(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def probe(name, A, blockings, passes):
    import scipy.sparse as sp
    import torch
    import deeppreconditioning_amd as D
    from oracle import oracle as O
    A = sp.csr_matrix(A, dtype="float64")
    A.sort_indices()
    n = A.shape[0]
    b = torch.from_numpy(O.rhs(n, 0)).cuda()
    cases = {"jacobi": D.Jacobi(), "ic0 multicolour solve": D.IC0("solve", ordering="multicolor"), "ic0 caller's order solve": D.IC0("solve")}
    for label, blocks in blockings.items():
        for variant in ("ic0", "dic"):
            cases[f"block {variant}, {label}"] = D.BlockIC(blocks=blocks, variant=variant)
    handles, rows = {}, {}
    for key, M in cases.items():
        S = D.CsrSystem.from_any(A, reorder=None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(M)
        torch.cuda.synchronize()
        rows[key] = {"setup_ms": round(1e3 * (time.perf_counter() - t0), 3), "precond_nnz": S.info()["precond_nnz"]}
        if key.startswith("block"):
            bi = S.block_ic_info()
            rows[key].update(blocks=bi["blocks"], max_block=bi["max_block"], levels_lower=bi["levels_lower"], levels_upper=bi["levels_upper"],
                             threads=bi["threads"])
            S.update_values(A.data)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.set_preconditioner(M)
            torch.cuda.synchronize()
            rows[key]["reattach_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            assert S.block_ic_info()["pattern_reused"]
            nnz = rows[key]["precond_nnz"]
            rows[key]["apply_bytes"] = 2 * 10 * (nnz - n) + n * (2 * 8 + 2 * 2 + 2 * 4 + 3 * 8 + 4)
        S.solve(b, rtol_sq=1e-8, max_iter=1024)              # warm-up (graph capture, code objects)
        S.precond_apply(b)
        handles[key] = S
    apply_us = {k: [] for k in cases}
    update_us = {k: [] for k in cases}
    solve_ms = {k: [] for k in cases}
    for _ in range(passes):
        for key, S in handles.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                S.precond_apply(b)
            torch.cuda.synchronize()
            apply_us[key].append(1e6 * (time.perf_counter() - t0) / 20)
            t0 = time.perf_counter()
            res = S.solve(b, rtol_sq=1e-8, max_iter=1024)
            solve_ms[key].append(1e3 * (time.perf_counter() - t0))
            update_us[key].append(1e6 * res.seconds / max(1, res.iterations))
            rows[key].update(iterations=res.iterations, converged=res.status == 0)
    for key in cases:
        rows[key].update(apply_us=_med(apply_us[key]), update_us=_med(update_us[key]), solve_ms=_med(solve_ms[key]))
        if "apply_bytes" in rows[key]:
            rows[key]["apply_gbs"] = round(rows[key]["apply_bytes"] / (rows[key]["apply_us"]["median"] * 1e-6) / 1e9, 1)
        print(name, key, rows[key], file=sys.stderr, flush=True)
        handles[key].close()
    return {"system": name, "rows": n, "nnz": int(A.nnz), "stream_gbs": round(D.operators.stream_bench(), 1), "passes": passes, "cases": rows}


def render(path):
    def spread(c):
        return f"{c['median']} ({c['min']} .. {c['max']})"
    for r in (json.loads(line) for line in open(path)):
        print(f"### {r['system']}: {r['rows']} rows, {r['nnz']} entries; medians of {r['passes']} alternating passes (min .. max); "
              f"streaming kernel {r['stream_gbs']} GB/s\n")
        print("| preconditioner | blocks | largest | levels L / L^T | threads | setup ms | re-attach ms | us / apply | apply GB/s | updates | us / update | ms to 1e-8 |")
        print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
        for k, c in r["cases"].items():
            lv = f"{c['levels_lower']} / {c['levels_upper']}" if "levels_lower" in c else ""
            its = f"{c['iterations']}" + ("" if c["converged"] else " (not converged)")
            print(f"| {k} | {c.get('blocks', '')} | {c.get('max_block', '')} | {lv} | {c.get('threads', '')} | {c['setup_ms']} | {c.get('reattach_ms', '')} | "
                  f"{spread(c['apply_us'])} | {c.get('apply_gbs', '')} | {its} | {spread(c['update_us'])} | {spread(c['solve_ms'])} |")
        print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="poisson2d_256,poisson3d_100,quadtree_1m")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--render", default=None)
    a = ap.parse_args()
    if a.render:
        render(a.render)
        return
    if a.passes < 5:
        ap.error("at least 5 passes")
    out = open(a.out, "w") if a.out else sys.stdout
    for name, A, blockings in _systems(a.systems.split(",")):
        out.write(json.dumps(probe(name, A, blockings, a.passes)) + "\n")
        out.flush()


if __name__ == "__main__":
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    main()
