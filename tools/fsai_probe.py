"""FSAI (dpcg_set_precond_fsai) against Jacobi and the incomplete-Cholesky factors: setup, cost of an update, time to solution.

    python tools/fsai_probe.py --out profiles/fsai_probe.jsonl
    python tools/fsai_probe.py --render profiles/fsai_probe.jsonl          # the tables of profiles/fsai_probe.md

Per system: for FSAI(1) and FSAI(2) the first attach (symbolic + numeric phase + the factor's SpMV plans) and the re-attach after
update_values (numeric phase + plans only), in ms, median of 3 after one warm-up of the kernels on a second handle; beside them
the setup of IC0("multiply") and ICholT("multiply") on the same system (ICholT only up to --icholt-max-rows rows: one wave walks
its columns).  For FSAI(1), FSAI(2), Jacobi and IC0("solve", ordering="multicolor"): iterations, us per PCG update (dpcg_solve's
own timer over the updates), ms to solution (rtol_sq = 1e-8, max_iter = 1024; the solve alone, median of 5 after a warm-up) and the
form the solve took (one launch by the whole chip, or launches).  The probe runs with DPCG_SETUP_TRACE=1 and reads the library's own
phase times from stderr: "fsai: symbolic", "fsai: numeric" and the rest of the attach (transposition, SpMV plans).  For level 1 the
numeric phase is set against the streaming ceiling `stream_bench` measures on the same box: least bytes = 4 per gather-map entry
+ 8 per entry of tril(A) + 8 per entry of L + 12 per column.
"""

import argparse
import json
import os
import re
import tempfile
import statistics
import sys
import time


def _systems(names):
    from deeppreconditioning_amd import meshes
    from oracle import oracle as O
    make = {
        "poisson2d_256": lambda: O.poisson2d(256),
        "poisson2d_512": lambda: O.poisson2d(512),
        "poisson2d_1024": lambda: O.poisson2d(1024),
        "poisson3d_64": lambda: O.poisson3d(64),
        "poisson3d_100": lambda: O.poisson3d(100),
        "quadtree_1m": lambda: meshes.quadtree_fv_laplacian(1000, 5),
    }
    for name in names:
        yield name, make[name]()


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _phases(fn):
    """Run fn with stderr (the C library's too) captured; ms by phase name of the library's setup trace."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            wall = _timed(fn)
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read()
    out = {}
    for name, ms in re.findall(r"\[dpcg setup\] (.+?)\s+([0-9.]+) ms", text):
        out[name.strip()] = out.get(name.strip(), 0.0) + float(ms)
    return wall, out


def _fsai_setups(D, A, level):
    """(first attach, re-attach after update_values) in ms: medians of 3; every first attach on a fresh handle."""
    warm = D.CsrSystem.from_any(A, reorder=None)
    warm.set_preconditioner(D.FSAI(level=level))
    warm.close()
    first, again, symbolic, numeric = [], [], [], []
    for _ in range(3):
        S = D.CsrSystem.from_any(A, reorder=None)
        wall, ph = _phases(lambda: S.set_preconditioner(D.FSAI(level=level)))
        first.append(wall)
        symbolic.append(ph.get("fsai: symbolic", float("nan")))
        S.update_values(A.data)
        wall, ph = _phases(lambda: S.set_preconditioner(D.FSAI(level=level)))
        again.append(wall)
        numeric.append(ph.get("fsai: numeric", float("nan")))
        assert S.fsai_info()["pattern_reused"] and "fsai: symbolic" not in ph
        S.close()
    return statistics.median(first), statistics.median(again), statistics.median(symbolic), statistics.median(numeric)


def _setup_ms(S, make):
    S.set_preconditioner(make())
    return statistics.median(_timed(lambda: S.set_preconditioner(make())) for _ in range(3))


def _solve(S, b):
    import torch
    S.solve(b, rtol_sq=1e-8, max_iter=1024)          # warm-up (graph capture, code objects)
    walls, per = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = S.solve(b, rtol_sq=1e-8, max_iter=1024)
        walls.append(time.perf_counter() - t0)
        per.append(res.seconds / max(1, res.iterations))
    return {"iterations": res.iterations, "converged": res.status == 0, "solve_ms": round(1e3 * statistics.median(walls), 3),
            "us_per_update": round(1e6 * statistics.median(per), 2),
            "form": "one launch" if S.chip_info()["chip_by_default"] else "launches"}


def probe(name, A, icholt_max_rows):
    import scipy.sparse as sp
    import torch
    import deeppreconditioning_amd as D
    from oracle import oracle as O
    A = sp.csr_matrix(A, dtype="float64")
    A.sort_indices()
    n = A.shape[0]
    b = torch.from_numpy(O.rhs(n, 0)).cuda()
    row = {"system": name, "rows": n, "nnz": int(A.nnz)}
    S = D.CsrSystem.from_any(A, reorder=None)
    ceiling = D.operators.stream_bench()             # GB/s of the library's own streaming kernel on this box
    for level in (1, 2):
        first, again, symbolic, numeric = _fsai_setups(D, A, level)
        S.set_preconditioner(D.FSAI(level=level))
        info = S.fsai_info()
        out = {"setup_ms": round(first, 3), "reattach_ms": round(again, 3), "symbolic_ms": round(symbolic, 3), "numeric_ms": round(numeric, 3),
               "precond_nnz": S.info()["precond_nnz"], "max_m": info["max_m"]}
        if level == 1:                               # the numeric phase against the streaming ceiling
            import numpy as np
            mi = np.diff(sp.triu(A, format="csr").indptr)
            tri = np.where(mi <= 4, 10, np.where(mi <= 8, 36, mi * (mi + 1) // 2))
            least = 4 * int(tri.sum()) + 8 * int(sp.tril(A).nnz) + 8 * out["precond_nnz"] + 12 * n
            out["numeric_gbs"] = round(least / (numeric * 1e-3) / 1e9, 1)
            out["stream_gbs"] = round(ceiling, 1)
            out["numeric_share_of_stream"] = round(out["numeric_gbs"] / ceiling, 3)
        out.update(_solve(S, b))
        row[f"fsai_{level}"] = out
        print(name, f"fsai_{level}", out, file=sys.stderr, flush=True)
    cases = {"jacobi": lambda: D.Jacobi(), "ic0_multicolor_solve": lambda: D.IC0("solve", ordering="multicolor")}
    for key, make in cases.items():
        out = {"setup_ms": round(_setup_ms(S, make), 3), "precond_nnz": S.info()["precond_nnz"]}
        out.update(_solve(S, b))
        row[key] = out
        print(name, key, out, file=sys.stderr, flush=True)
    yard = {"ic0_multiply": lambda: D.IC0("multiply")}
    if n <= icholt_max_rows:
        yard["icholt_multiply"] = lambda: D.ICholT("multiply")
    for key, make in yard.items():                   # setup only: the yardstick of the FSAI setup
        row[key] = {"setup_ms": round(_setup_ms(S, make), 3), "precond_nnz": S.info()["precond_nnz"]}
        print(name, key, row[key], file=sys.stderr, flush=True)
    S.close()
    return row


def render(path):
    rows = [json.loads(line) for line in open(path)]
    print("| system | rows | preconditioner | setup ms | of it symbolic | re-attach ms | of it numeric | nnz(factor) | max m | iterations | us / update | solve ms | form |")
    print("|---|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|")
    for r in rows:
        for k in [k for k in r if isinstance(r[k], dict)]:
            c = r[k]
            its = "" if "iterations" not in c else f"{c['iterations']}" + ("" if c["converged"] else " (not converged)")
            print(f"| {r['system']} | {r['rows']} | {k} | {c['setup_ms']} | {c.get('symbolic_ms', '')} | {c.get('reattach_ms', '')} | {c.get('numeric_ms', '')} | "
                  f"{c['precond_nnz']} | {c.get('max_m', '')} | "
                  f"{its} | {c.get('us_per_update', '')} | {c.get('solve_ms', '')} | {c.get('form', '')} |")
    print()
    print("| system | level-1 numeric ms | least bytes / time, GB/s | stream_bench GB/s | share |")
    print("|---|---:|---:|---:|---:|")
    for r in rows:
        c = r["fsai_1"]
        print(f"| {r['system']} | {c['numeric_ms']} | {c['numeric_gbs']} | {c['stream_gbs']} | {c['numeric_share_of_stream']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="poisson2d_256,poisson2d_512,poisson3d_64,poisson3d_100,quadtree_1m")
    ap.add_argument("--icholt-max-rows", type=int, default=70000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--render", default=None)
    a = ap.parse_args()
    if a.render:
        render(a.render)
        return
    out = open(a.out, "w") if a.out else sys.stdout
    for name, A in _systems(a.systems.split(",")):
        out.write(json.dumps(probe(name, A, a.icholt_max_rows)) + "\n")
        out.flush()


if __name__ == "__main__":
    os.environ["DPCG_SETUP_TRACE"] = "1"             # (read once by the library: before its first setup)
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    main()
