"""The projected initial guess (`ProjectedGuess`, dpcg_guess_*) on a time-stepping sequence: what it saves and what it costs.

    python tools/guess_probe.py --out profiles/guess_probe.md

Per size (256 x 256 = 65 536 and 1024 x 1024 = 1 048 576 rows): the sequence of tests/test_guess_gpu.py::test_changing_matrix --
A_t = D_t^1/2 A D_t^1/2 + 0.05 I with a drifting coefficient field, a smoothly varying right-hand side, `update_values` every
step, Jacobi attached again every step, rtol_sq = 1e-16 -- run with and without the guess:
  * PCG updates per step, with and without;
  * wall time of project, of update and of the re-orthonormalisation (the project after `update_values` minus a second project
    of the same b), from instrumented passes of their own, each at the largest basis the sequence reached (median, least and
    most over the repeats), beside the time the measured streaming rate
    (`stream_bench` over the same number of bytes) gives for the bytes the call has to move -- l columns of n doubles:
    project 2 l n 8 (dot products, combination), update 6 l n 8 (two Gram-Schmidt passes: X~ once for the dot products, X~ and
    W for the subtraction) plus the SpMV's 12 nnz + 16 n, re-orthonormalisation 2 (l^2 + 4 l) n 8 (two rounds: the Gram matrix
    column by column, X~ and W read and written by the triangular multiply) plus l SpMVs;
  * time to solution of the whole sequence, everything included (update_values, Jacobi, project, solve, update): --repeats
    passes of each variant, alternating and swapping who goes first; median, least and most.
"""

import argparse
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp


def grid_poisson(m):
    t = sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    A = sp.csr_matrix(sp.kron(sp.identity(m), t) + sp.kron(t, sp.identity(m)))
    A.sort_indices()
    return A


class Sequence:
    def __init__(self, m):
        self.m, self.A0 = m, grid_poisson(m)
        xs = (np.arange(m) + 0.5) / m
        self.xg, self.yg = np.meshgrid(xs, xs, indexing="xy")
        self.rows = np.repeat(np.arange(m * m), np.diff(self.A0.indptr))
        self.diag = self.rows == self.A0.indices

    def step(self, t):
        xg, yg = self.xg, self.yg
        s = np.sqrt(1.0 + 0.5 * np.sin(2 * np.pi * (xg - 0.02 * t)) * np.cos(2 * np.pi * yg)).ravel()
        data = s[self.rows] * self.A0.data * s[self.A0.indices] + 0.05 * self.diag
        b = (np.sin(np.pi * xg) * np.sin(np.pi * yg) * (1 + 0.1 * t) + 0.3 * np.sin(2 * np.pi * (xg + 0.03 * t)) * yg).ravel()
        return data, b


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def stream_ms(nbytes):
    from deeppreconditioning_amd import operators as ops
    out_bytes = max(1 << 20, int(nbytes) // 3 // 4096 * 4096)
    gbs = ops.stream_bench(n_read=2, write=True, out_bytes=out_bytes, repeats=20)
    return nbytes / (gbs * 1e9) * 1e3, gbs


def one_sequence(D, A1, inputs, depth, mode):
    """One pass over the sequence.  mode "without" | "with": nothing but what a caller would do, timed as a whole;
    "instrumented": project twice (the first one carries the re-orthonormalisation) and every call timed by itself."""
    import torch
    S = D.CsrSystem.from_any(A1)
    g = D.ProjectedGuess(S, depth=depth) if mode != "without" else None
    iters, t_proj, t_upd, t_reo = [], [], [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for data, b in inputs:
        bv = torch.from_numpy(b).cuda()
        S.update_values(data)
        S.set_preconditioner(D.Jacobi())
        if mode != "instrumented":
            iters.append(S.solve(bv, rtol_sq=1e-16, max_iter=20000, want_history=False, guess=g).iterations)
            continue
        ms_first, x0 = timed(lambda: g.project(bv))
        ms_second, x0 = timed(lambda: g.project(bv))
        l = g.info()["size"]
        r = S.solve(bv, x0, rtol_sq=1e-16, max_iter=20000, want_history=False)
        ms_update, _ = timed(lambda: g.update(r.x))
        t_proj.append((l, ms_second))
        t_reo.append((l, ms_first - ms_second))
        if l < depth:                          # (a full basis restarts: one SpMV, no Gram-Schmidt pass)
            t_upd.append((l, ms_update))
    torch.cuda.synchronize()
    total = 1e3 * (time.perf_counter() - t0)
    info = g.info() if g else None
    S.close()
    return dict(iters=iters, total_ms=total, proj=t_proj, upd=t_upd, reo=t_reo, info=info)


def spread(v):
    return f"{statistics.median(v):.1f} ms (median of {len(v)}; {min(v):.1f} .. {max(v):.1f})"


def run(m, depth, steps, repeats, out):
    import deeppreconditioning_amd as D
    seq = Sequence(m)
    n, nnz = m * m, seq.A0.nnz
    inputs = [seq.step(t) for t in range(1, steps + 1)]
    A1 = sp.csr_matrix((inputs[0][0], seq.A0.indices, seq.A0.indptr), shape=(n, n))
    for mode in ("with", "without", "instrumented"):          # warm-up: kernels loaded, the block cache filled
        one_sequence(D, A1, inputs[:3], depth, mode)
    totals = {"without": [], "with": []}
    last = {}
    for rep in range(repeats):                                 # alternating, and alternating who goes first
        for mode in (("without", "with") if rep % 2 == 0 else ("with", "without")):
            last[mode] = one_sequence(D, A1, inputs, depth, mode)
            totals[mode].append(last[mode]["total_ms"])
    proj, upd, reo = [], [], []
    for rep in range(repeats):
        r = one_sequence(D, A1, inputs, depth, "instrumented")
        proj += r["proj"]
        upd += r["upd"]
        reo += r["reo"]
    w, wo = last["with"], last["without"]
    col = n * 8
    print(f"\n## {m} x {m} = {n} rows, depth {depth}, {steps} steps\n", file=out)
    print(f"- PCG updates per step without the guess: {wo['iters']} (sum {sum(wo['iters'])})", file=out)
    print(f"- PCG updates per step with the guess:    {w['iters']} (sum {sum(w['iters'])}, {sum(wo['iters']) / max(1, sum(w['iters'])):.2f} x fewer)", file=out)
    print(f"- basis at the end: {w['info']}", file=out)
    print(f"- whole sequence, everything included, {repeats} alternating repeats: without {spread(totals['without'])}, "
          f"with {spread(totals['with'])}\n", file=out)
    print("| call | columns l | samples | measured ms: median (min .. max) | bytes | ms at the streaming rate | GB/s of stream_bench | median / streaming |", file=out)
    print("|---|---|---|---|---|---|---|---|", file=out)
    for name, samples, nbytes_of in (("project", proj, lambda l: 2 * l * col),
                                     ("update (appends)", upd, lambda l: 6 * l * col + 12 * nnz + 16 * n),
                                     ("re-orthonormalisation", reo, lambda l: 2 * (l * l + 4 * l) * col + l * (12 * nnz + 16 * n))):
        l = max(k for k, _ in samples)
        at = [ms for k, ms in samples if k == l]
        med = statistics.median(at)
        nbytes = nbytes_of(l)
        ideal, gbs = stream_ms(nbytes)
        print(f"| {name} | {l} | {len(at)} | {med:.3f} ({min(at):.3f} .. {max(at):.3f}) | {nbytes} | {ideal:.3f} | {gbs:.0f} | {med / ideal:.1f} |", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else sys.stdout
    print("# `tools/guess_probe.py`: the projected initial guess on a time-stepping sequence (one MI355X)", file=out)
    print("\nWall times around the Python calls, device-synchronised.  The whole-sequence times come from passes that do nothing but "
          "what a caller does (`solve(b, guess=guess)`), the two variants alternating; the per-call times from separate passes "
          "that project twice per step.  An update of a full basis is a restart (one SpMV, no Gram-Schmidt pass) and is not in "
          "the update row.", file=out)
    for m in args.sizes:
        run(m, args.depth, args.steps, args.repeats, out)
    if args.out:
        out.close()


if __name__ == "__main__":
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    main()
