"""ILUT (dpcg_set_precond_ilut) against Jacobi and ICholT("multiply"): setup, cost of an update, time to solution.

    python tools/ilut_probe.py --out profiles/ilut_probe.jsonl
    python tools/ilut_probe.py --render profiles/ilut_probe.jsonl          # the tables of profiles/ilut_probe.md

Per system (the reference's sizes -- poisson2d(48), 2.3K rows, and a quadtree mesh of 22.8K rows -- and a 262K-row grid): the
setup in ms (median of 3 attaches, after one warm-up; the factorisation is one wave walking the rows), the factor's nnz, and for
Jacobi, ICholT("multiply") and ILUT in both modes (add_fill_in=1, threshold=0.1, the harness's arguments, and whatever --params
adds: ilut_<mode>_p<fill>_t<threshold>) the iterations, the
us per PCG update (dpcg_solve's own timer over the updates) and ms to solution (rtol_sq = 1e-8, max_iter = 1024, the reference's
defaults; setup + solve wall time).
"""

import argparse
import json
import statistics
import sys
import time


def _systems(names):
    from deeppreconditioning_amd import meshes
    from oracle import oracle as O
    make = {
        "poisson2d_48": lambda: O.poisson2d(48),
        "quadtree_150": lambda: meshes.quadtree_fv_laplacian(150, 5),
        "poisson2d_512": lambda: O.poisson2d(512),
    }
    for name in names:
        yield name, make[name]()


def _setup_ms(S, make):
    import torch
    S.set_preconditioner(make())
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.set_preconditioner(make())
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def _solve(S, b):
    import torch
    S.solve(b, rtol_sq=1e-8, max_iter=1024)          # warm-up (graph capture, code objects)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = S.solve(b, rtol_sq=1e-8, max_iter=1024)
    wall = time.perf_counter() - t0
    return {"iterations": res.iterations, "converged": res.status == 0, "solve_ms": round(1e3 * wall, 3),
            "us_per_update": round(1e6 * res.seconds / max(1, res.iterations), 2)}


def probe(name, A, params):
    import torch
    import deeppreconditioning_amd as D
    from oracle import oracle as O
    S = D.CsrSystem.from_any(A, reorder=None)
    n = S.n
    b = torch.from_numpy(O.rhs(n, 0)).cuda()
    row = {"system": name, "rows": n, "nnz": int(A.nnz)}
    cases = {
        "jacobi": lambda: D.Jacobi(),
        "icholt_multiply": lambda: D.ICholT("multiply"),
    }
    for fill, thr in params:
        tag = "" if (fill, thr) == (1, 0.1) else f"_p{fill}_t{thr:g}"
        for mode in ("multiply", "solve"):
            cases[f"ilut_{mode}{tag}"] = (lambda m=mode, f=fill, t=thr: D.ILUT(m, add_fill_in=f, threshold=t))
    for key, make in cases.items():
        setup = _setup_ms(S, make)
        out = {"setup_ms": round(setup, 3), "precond_nnz": S.info()["precond_nnz"]}
        out.update(_solve(S, b))
        out["ms_to_solution"] = round(setup + out["solve_ms"], 3)
        row[key] = out
        print(name, key, out, file=sys.stderr, flush=True)
    S.close()
    return row


def render(path):
    rows = [json.loads(line) for line in open(path)]
    print("| system | rows | preconditioner | setup ms | nnz(M factors) | iterations | us / update | ms to solution |")
    print("|---|---:|---|---:|---:|---:|---:|---:|")
    for r in rows:
        for k in [k for k in r if isinstance(r[k], dict)]:
            c = r[k]
            its = f"{c['iterations']}" + ("" if c["converged"] else " (not converged)")
            print(f"| {r['system']} | {r['rows']} | {k} | {c['setup_ms']} | {c['precond_nnz']} | {its} | {c['us_per_update']} | "
                  f"{c['ms_to_solution']} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="poisson2d_48,quadtree_150,poisson2d_512")
    ap.add_argument("--params", default="1:0.1", help="ILUT add_fill_in:threshold pairs, comma-separated (1:0.1: the harness's)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--render", default=None)
    a = ap.parse_args()
    if a.render:
        render(a.render)
        return
    out = open(a.out, "w") if a.out else sys.stdout
    for name, A in _systems(a.systems.split(",")):
        params = [(int(f), float(t)) for f, t in (p.split(":") for p in a.params.split(","))]
        out.write(json.dumps(probe(name, A, params)) + "\n")
        out.flush()


if __name__ == "__main__":
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    main()
