"""Mixed-precision PCG (dpcg_solve_refined, dpcg_refine.hip): what the count test may allow, and whether the solve pays.

    python tools/refine_probe.py --cpu-spread      # no GPU: the section "Count margin" of profiles/refine_probe.md
    python tools/refine_probe.py                   # on the GPU: the section "Time to the solution"
    python tools/refine_probe.py --edges           # profiles/refine_edges.md: the CPU sections, and the device's where there is a GPU

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
EDGES_PROFILE = ROOT / "profiles" / "refine_edges.md"
REPEATS = 5


def write_section(tag, lines, PROFILE=PROFILE, title="# Mixed-precision PCG (dpcg_solve_refined)\n"):
    """replace (or append) one section of the profile, leaving the other as it is"""
    text = PROFILE.read_text() if PROFILE.exists() else title
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


def edges():
    """profiles/refine_edges.md: what tests/test_refine_edges_host.py asserts and tests/test_refine_edges_gpu.py compares, as figures"""
    import refine_edge_cases as C
    title = "# Mixed-precision PCG at its edges (tests/test_refine_edges_*.py)\n"
    put = lambda tag, lines: write_section(tag, lines, EDGES_PROFILE, title)
    lines = ["## Short runs: CPU spread and tolerance", "", "`python tools/refine_probe.py --edges`.  One inner solve of t updates "
             "(`max_iter=t, rtol_sq=1e-30, inner_rtol_sq=1e-300`, x0 = None), the numpy restatement as it stands against itself with "
             + ", ".join(C.PERTURBATIONS) + ": the largest per-entry spread of x in fp32 ulps of ||x||_inf and of a history entry, "
             "relatively, over both preconditioners and t = 1, 2, 3.  The device may differ by twice the spread, at least by the floor "
             f"(1 ulp; {C.HIST_FLOOR:.3g} = 2^-22).", "",
             "| system | rows | lanes per row | spread of x (ulp) | spread of the history | tolerance of x (ulp) | tolerance of the history |",
             "|---|---|---|---|---|---|---|"]
    for name in C.SYSTEMS:
        A, _ = C.system(name)
        got = [C.measure_spread(name, pre, t) for pre in C.PRES for t in C.TS]
        sx, sh = max(g[0] for g in got), max(g[1] for g in got)
        lines.append(f"| {name} | {A.shape[0]} | {C.lanes_per_row(A)} | {sx:.3g} | {sh:.3g} | {max(2 * sx, 1.0):.3g} | {max(2 * sh, C.HIST_FLOOR):.3g} |")
    lines += ["", "No perturbation flips an fp32 rounding in runs this short: every spread is that of the fp64 scalars alone, and the floors are "
              "the tolerances."]
    put("cpu spread", lines)
    lines = ["## Mutants: one entry of A32 set to zero", "", "Distance of the mutated restatement from the true one over the tolerance of x, "
             "at t = 1, 2, 3 (the test asks >= 10 at t = 2 and 3; `-`: the system has no such entry).", "",
             "| system | M | " + " | ".join(C.MUTANTS) + " |", "|---|---|---|---|---|"]
    for name in C.SYSTEMS:
        for pre in C.PRES:
            cells = []
            for which in C.MUTANTS:
                f = [C.mutant_factor(name, pre, t, which) for t in C.TS]
                cells.append("-" if f[0] is None else ", ".join(f"{v:.3g}" for v in f))
            lines.append(f"| {name} | {pre} | " + " | ".join(cells) + " |")
    put("mutants", lines)
    lines = ["## Stagnation candidates", "", "M = I, rtol_sq = 1e-30, b = default_rng(1).random(n); a candidate qualifies when it ends "
             "\"stagnated\" after at least one productive outer step with every outer margin and the stop's own margin, "
             "rr / (0.25 rr_prev), >= 1.2.", "",
             "| system | reason | outer steps | updates | smallest outer margin | margin of the stop | outer history | qualifies |", "|---|---|---|---|---|---|---|---|"]
    for name in C.STAGNATION_CANDIDATES:
        _, _, run = C.stagnation_run(name)
        margin = min(run["outer_margins"]) if run["outer_margins"] else 0.0
        lines.append(f"| {name} | {run['reason']} | {run['outer_steps']} | {run['iterations']} | {margin:.3g} | {C.stagnation_margin(run):.3g} | "
                     + ", ".join(f"{h:.2e}" for h in run["outer_history"]) + f" | {'yes' if C.qualifies_as_stagnation(run) else 'no'} |")
    lines += ["", "Stop cases (tests/refine_edge_cases.py, `stop_cases`): the restatement's status, updates, outer steps and smallest outer margin.", "",
              "| case | status | updates | outer steps | reason | smallest outer margin |", "|---|---|---|---|---|---|"]
    for case in C.stop_cases():
        r = C.stop_restated(case)
        lines.append(f"| {case} | {r['status']} | {r['iterations']} | {r['outer_steps']} | {r['reason']} | "
                     + (f"{min(r['outer_margins']):.3g}" if r["outer_margins"] else "-") + " |")
    lines += ["", f"Power-of-two scalings of {C.SCALING_SYSTEM}: (k, m) = {C.SCALINGS} leave the restatement's x 2^(m-k) x, counts and histories "
              "bit for bit; k = 60 was not shrunk."]
    put("stops", lines)
    try:
        import torch
        have = torch.cuda.is_available()
    except ImportError:
        have = False
    if not have:
        print(f"no GPU: the section of the device's distances in {EDGES_PROFILE} is left as it is")
        return
    import deeppreconditioning_amd as D
    lines = ["## The device against the restatement", "", f"`python tools/refine_probe.py --edges` on {torch.cuda.get_device_properties(0).gcnArchName}: "
             "per-entry distance of `solve_refined`'s x (fp32 ulps of ||x||_inf) and of its inner history (relative) from the restatement.", "",
             "| system | M | t | lanes per row | distance of x (ulp) | distance of the history |", "|---|---|---|---|---|---|"]
    wx = wh = 0.0
    for name, pre, t in C.SHORT_CASES:
        A, b = C.system(name)
        ref = C.short_run(name, pre, t)
        S = D.CsrSystem.from_any(A, reorder=None)
        S.set_preconditioner(D.Jacobi() if pre == "jacobi" else None)
        res = S.solve_refined(torch.from_numpy(b).cuda(), **C.short_kwargs(t))
        dx, dh = C.x_distance(res.x.cpu().numpy(), ref["x"], b), C.hist_distance(res.res_history, ref["res_history"])
        wx, wh = max(wx, dx), max(wh, dh)
        lines.append(f"| {name} | {pre} | {t} | {C.lanes_per_row(A)} | {dx:.3g} | {dh:.3g} |")
    lines += ["", f"Largest: **{wx:.3g} ulp** of x, **{wh:.3g}** of a history entry: the device's sums, formed in another order, flip no fp32 "
              "rounding in these runs either."]
    put("device", lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-spread", action="store_true")
    ap.add_argument("--edges", action="store_true")
    args = ap.parse_args()
    edges() if args.edges else cpu_spread() if args.cpu_spread else gpu_timing()
