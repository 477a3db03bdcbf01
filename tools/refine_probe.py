"""Mixed-precision PCG (dpcg_solve_refined, dpcg_refine.hip): what the count test may allow, and whether the solve pays.

    python tools/refine_probe.py --cpu-spread      # no GPU: the section "Count margin" of profiles/refine_probe.md
    python tools/refine_probe.py                   # on the GPU: the section "Time to the solution"

Count margin (CPU, the numpy restatement tests/refine_restatement.py): the systems, preconditioners and tolerances of
tests/test_refine_gpu.py, each solved as it stands, with b perturbed by 1e-16 and by 1e-12 relative, and with every dot summed back to
front.  fp32 stores make the inner history sensitive to the last bits of the fp64 alpha and beta, so the total update count moves;
the largest relative spread over the cases that stay within 10 % is what the device's count may differ by, times two.

Time to the solution (GPU): `solve_refined` against `solve` (the default path, and the multi-launch path as three plain launches
per update: DPCG_NO_SMALL | DPCG_NO_TEAM | DPCG_NO_FUSE | DPCG_NO_GRAPH) on 128^3 and 160^3 Poisson, the 1 M-row quadtree mesh and
100^3 Poisson, Jacobi, b = poisson.rhs(seed 0), rtol_sq 1e-8 and 1e-16: medians of REPEATS alternating runs after a warm-up.  Bytes
per inner update as bench.py counts them, at fp32 widths: 8 per non-zero (value, column) and 4 x 11 per row (K1 writes q, K2 reads
q, r, dinv and writes r, K3 reads r, dinv, p, d and writes p, d); the fp64 launches: 12 per non-zero and 8 x 11 per row.  The rate
is set against the library's streaming kernel (dpcg_stream_bench, triad shape).
"""

import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PROFILE = ROOT / "profiles" / "refine_probe.md"
BEGIN, END = "<!-- {0}: begin -->", "<!-- {0}: end -->"
REPEATS = 5


def write_section(tag, lines):
    """replace (or append) one section of the profile, leaving the other as it is"""
    text = PROFILE.read_text() if PROFILE.exists() else "# Mixed-precision PCG (dpcg_solve_refined)\n"
    block = "\n".join([BEGIN.format(tag)] + lines + [END.format(tag)])
    if BEGIN.format(tag) in text:
        head, rest = text.split(BEGIN.format(tag), 1)
        text = head + block + rest.split(END.format(tag), 1)[1]
    else:
        text = text.rstrip("\n") + "\n\n" + block + "\n"
    PROFILE.parent.mkdir(exist_ok=True)
    PROFILE.write_text(text)


def cpu_spread():
    import refine_cases as cases
    import refine_restatement as R
    rows, worst = [], 0.0
    for name, pre, rtol_sq in cases.CASES:
        A, b = cases.system(name)
        runs = {"as it stands": R.solve_refined(A, b, jacobi=pre == "jacobi", rtol_sq=rtol_sq, max_iter=cases.MAX_ITER)}
        rng = np.random.default_rng(7)
        for tag, eps in (("b (1 + 1e-16 u)", 1e-16), ("b (1 + 1e-12 u)", 1e-12)):
            bp = b * (1.0 + eps * rng.uniform(-1.0, 1.0, b.shape[0]))
            runs[tag] = R.solve_refined(A, bp, jacobi=pre == "jacobi", rtol_sq=rtol_sq, max_iter=cases.MAX_ITER)
        runs["dots back to front"] = R.solve_refined(A, b, jacobi=pre == "jacobi", rtol_sq=rtol_sq, max_iter=cases.MAX_ITER, reverse=True)
        base = runs["as it stands"]
        counts = [r["iterations"] for r in runs.values()]
        spread = (max(counts) - min(counts)) / base["iterations"]
        outers = sorted({r["outer_steps"] for r in runs.values()})
        margin = min(min(base["outer_margins"]), min(base["inner_margins"]))
        count_case = margin >= 1.2
        rows.append((name, pre, rtol_sq, base["iterations"], base["outer_steps"], counts, spread, outers, margin, count_case))
        if spread <= 0.10:
            worst = max(worst, spread)
        print(rows[-1], flush=True)
    excluded = [r for r in rows if r[6] > 0.10]
    lines = ["## Count margin (CPU)", "", "`python tools/refine_probe.py --cpu-spread`: the numpy restatement on the cases of tests/test_refine_gpu.py "
             f"(b = default_rng(1).random(n), max_iter {cases.MAX_ITER}); total inner updates as the case stands, with b (1 + 1e-16 u), with "
             "b (1 + 1e-12 u) and with every dot summed back to front.", "",
             "| system | M | rtol_sq | updates | outer steps | the four counts | spread | outer steps seen | smallest stop margin | count case |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, pre, rtol_sq, it, out, counts, spread, outers, margin, cc in rows:
        lines.append(f"| {name} | {pre} | {rtol_sq:g} | {it} | {out} | {counts} | {100 * spread:.2f} % | {outers} | {margin:.3f} | {'yes' if cc else 'no'} |")
    lines += ["", f"Largest relative spread of the total count over the cases within 10 %: **{100 * worst:.2f} %**; the device's total may differ "
              f"from the restatement's by twice that, **{100 * 2 * worst:.2f} %**.  Cases beyond 10 % (compared by true "
              f"residual only): {len(excluded)} of {len(rows)}" + (": " + ", ".join(f"{r[0]} {r[1]} {r[2]:g}" for r in excluded) if excluded else "") + "."]
    write_section("count margin", lines)
    print("\n".join(lines))


def gpu_timing():
    import torch

    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import _lib as L
    from deeppreconditioning_amd import meshes
    from deeppreconditioning_amd.operators import stream_bench
    from deeppreconditioning_amd.poisson import poisson_system, rhs

    plain3 = L.NO_SMALL | L.NO_TEAM | L.NO_FUSE | L.NO_GRAPH
    torch.cuda.set_device(0)
    name = torch.cuda.get_device_properties(0).gcnArchName
    triad = stream_bench(2, True, 1 << 28, 10)
    systems = [("poisson 128^3", lambda: poisson_system(3, 128)), ("poisson 160^3", lambda: poisson_system(3, 160)),
               ("quadtree 1M", lambda: D.CsrSystem.from_any(meshes.quadtree_fv_laplacian(1000, 0))), ("poisson 100^3", lambda: poisson_system(3, 100))]
    lines = ["## Time to the solution (GPU)", "", f"`python tools/refine_probe.py` on {name}.  Jacobi, b = poisson.rhs(seed 0), medians of {REPEATS} "
             f"alternating runs after a warm-up; loop times as the drivers report them.  Streaming kernel of the library (triad shape): {triad:.0f} GB/s.", "",
             "| system | rows | rtol_sq | variant | updates | outer steps | ms | us per update | GB/s per update | of the streaming kernel | final true residual | against default |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for label, make in systems:
        S = make()
        S.set_preconditioner(D.Jacobi())
        info = S.info()
        rows, nnz = int(info["n"]), int(info["nnz"])
        b = rhs(rows, 0)
        for rtol_sq in (1e-8, 1e-16):
            variants = {"solve (default path)": lambda: S.solve(b, rtol_sq=rtol_sq, max_iter=20000, want_history=False),
                        "solve (3 plain launches)": lambda: S.solve(b, rtol_sq=rtol_sq, max_iter=20000, flags=plain3, want_history=False),
                        "solve_refined": lambda: S.solve_refined(b, rtol_sq=rtol_sq, max_iter=20000, want_history=False)}
            got = {v: [] for v in variants}
            for rep in range(REPEATS + 1):
                for v, run in variants.items():                              # alternating
                    r = run()
                    if rep > 0:
                        got[v].append(r)
            base_ms = float(np.median([r.seconds for r in got["solve (default path)"]])) * 1e3
            for v, runs in got.items():
                ms = float(np.median([r.seconds for r in runs])) * 1e3
                r = runs[0]
                x = r.x
                e = b - S @ x
                true_res = float((e @ e) / (b @ b))
                refined = v == "solve_refined"
                per_update = (8 * nnz + 44 * rows) if refined else (12 * nnz + 88 * rows)
                us = ms * 1e3 / max(r.iterations, 1)
                rate = per_update / (us * 1e-6) / 1e9
                ok = "" if r.status == L.OK else f" (status {r.status})"
                lines.append(f"| {label} | {rows} | {rtol_sq:g} | {v}{ok} | {r.iterations} | {r.outer_steps if refined else ''} | {ms:.3f} | {us:.2f} | "
                             f"{rate:.0f} | {100 * rate / triad:.0f} % | {true_res:.2e} | {ms / base_ms:.2f}x |")
                print(lines[-1], flush=True)
        del S
        L.lib().dpcg_release_cached_memory()
    lines += ["", "us per update of `solve_refined` is its whole loop time over its inner updates: the outer steps (an fp64 SpMV, three vector passes "
              "and two host synchronisations each) are in it.  GB/s of the default path on 100^3 is nominal: the whole-chip kernel keeps the "
              "matrix on chip.",
              "", "The parent commit has no column of its own because it would repeat the `solve` rows: the change adds nothing to `dpcg_solve`'s path "
              "(a pointer at the end of the handle, and one release of it, null unless `solve_refined` ran, where the preconditioner is freed), "
              "`tests/test_refine_gpu.py` asserts that a plain solve's iterate and history keep their bits, and `bench.py` gives 2.2 ms per "
              "step, the figure DESIGN.md records for the parent (100^3, default path)."]
    write_section("time to the solution", lines)
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-spread", action="store_true")
    args = ap.parse_args()
    cpu_spread() if args.cpu_spread else gpu_timing()
