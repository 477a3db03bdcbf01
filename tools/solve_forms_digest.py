#!/usr/bin/env python3
"""Digest of one solve per path through the host layer of dpcg_solve, dpcg_solve_batch and dpcg_solve_refined, for comparing two
builds bit for bit (needs the GPU).

Every sum in the solve kernels is added in a fixed order, so a solve is reproducible to the bit: a change that means to leave the
arithmetic alone -- a change to the host code that stages a call, picks its form and delivers its results -- must print the same
lines before and after.  Per case: iteration count, status, SHA-256 of res_history's bytes and of x's bytes (of the error history
and of outer_history where there is one; of every member's x in a batch).

    python tools/solve_forms_digest.py [--reps N]            # the library to load: DPCG_LIBRARY, else the tree's own

Cases, each at the smallest system the host path sends there, each with x0 = None and x0 = cos(i), at most 200 updates (a case
that stops at the cap is as good a digest as one that converges):
  one workgroup    35 rows (5 x 7): M = I, Jacobi, an explicit CSR M, L L^T multiplied; DPCG_INIT_CHECK_R once
  one team         4 160 rows (65 x 64, the first grid above the team's minimum), Jacobi
  whole chip       the cases of tools/chip_forms_digest.py (imported, not copied), and a reordered handle once
  launch path      DPCG_NO_SMALL on 1 600 rows (40 x 40), Jacobi: graph replay, DPCG_NO_GRAPH, with x_true / err_history, a
                   reordered handle
  refined          dpcg_solve_refined on 1 600 rows: M = I, Jacobi, a reordered handle
  batches          eight one-workgroup systems; nine team systems (a group of eight and one of one); three whole-chip systems; three
                   systems with IC(0) by triangular solves on two streams; DPCG_SINGLE_REDUCTION on two systems
--reps N adds `#time` lines for the launch-bound forms, where host overhead shows: wall `seconds` of the 35-row solve, the 4 160-row
team solve and the eight-system batch, min / median / max of N solves after 3 warm-ups.
A tool, not a test: it pins nothing for a change that means to alter the arithmetic.  One process, no retries.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import deeppreconditioning_amd as D  # noqa: E402
from deeppreconditioning_amd import _lib as L  # noqa: E402
from deeppreconditioning_amd.batch import solve_batch  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import oracle as O  # noqa: E402

from chip_forms_digest import chip_cases  # noqa: E402
from projected_forms_digest import csr32, dirichlet, sha  # noqa: E402

MAX_ITER = 200
SMALL, TEAM, LAUNCH = (5, 7), (65, 64), (40, 40)


def vectors(n, seed=1):
    b = torch.from_numpy(np.random.default_rng(seed).random(n)).cuda()
    x0 = torch.from_numpy(np.cos(np.arange(n, dtype=np.float64))).cuda()
    return b, (("x0=None", None), ("x0=cos", x0))


def system(A, precond, reorder=None):
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(precond)
    assert (reorder is None) or S.reordered
    return S


def report(name, res, extra=""):
    print("%s iterations=%d status=%d hist=%s x=%s%s" % (name, res.iterations, res.status, sha(np.asarray(res.res_history)),
                                                        sha(res.x.detach().cpu().numpy()), extra), flush=True)


def timed(name, reps, solve):
    """wall seconds as the library reports them: min / median / max of reps calls after 3 warm-ups"""
    if reps <= 0:
        return
    for _ in range(3):
        solve()
    sec = [solve() for _ in range(reps)]
    print("#time %s seconds_us min=%.2f median=%.2f max=%.2f reps=%d" % (name, 1e6 * min(sec), 1e6 * float(np.median(sec)), 1e6 * max(sec),
                                                                         reps), flush=True)


def singles(reps):
    A = dirichlet(SMALL)
    b, starts = vectors(A.shape[0])
    lower = CO.ic0(A)
    for kind, M in (("identity", D.Identity()), ("jacobi", D.Jacobi()), ("csr", D.CsrPreconditioner(csr32(lower @ lower.T))),
                    ("llt_multiply", D.LLtMultiply(lower))):
        S = system(A, M)
        for tag, x0 in starts:
            report("one_workgroup n=35 %s %s" % (kind, tag), S.solve(b, x0, max_iter=MAX_ITER))
        if kind == "jacobi":
            report("one_workgroup n=35 jacobi x0=cos init_check_r", S.solve(b, starts[1][1], max_iter=MAX_ITER, flags=L.INIT_CHECK_R))
            timed("one_workgroup n=35 jacobi x0=None", reps, lambda: S.solve(b, None, max_iter=MAX_ITER).seconds)
        S.close()
    A = dirichlet(TEAM)
    b, starts = vectors(A.shape[0])
    S = system(A, D.Jacobi())
    assert S.reduction_geometry()["team_by_default"], S.reduction_geometry()
    for tag, x0 in starts:
        report("team n=4160 jacobi %s" % tag, S.solve(b, x0, max_iter=MAX_ITER))
    report("team n=4160 jacobi x0=cos init_check_r", S.solve(b, starts[1][1], max_iter=MAX_ITER, flags=L.INIT_CHECK_R))
    timed("team n=4160 jacobi x0=None", reps, lambda: S.solve(b, None, max_iter=MAX_ITER).seconds)
    S.close()
    for name, A, precond, recurrence, max_iter in chip_cases():
        b, starts = vectors(A.shape[0])
        S = system(A, precond(A))
        assert S.chip_info()["chip_by_default"], (name, S.chip_info())
        for tag, x0 in starts:
            res = S.solve(b, x0, recurrence=recurrence, max_iter=min(max_iter, MAX_ITER))
            report("chip %s %s" % (name, tag), res, " recurrence=%s" % res.recurrence)
        if name == "standard_jacobi":
            report("chip %s x0=cos init_check_r" % name, S.solve(b, starts[1][1], max_iter=MAX_ITER, flags=L.INIT_CHECK_R))
        S.close()
    A = O.unstructured_like(O.poisson3d(41), seed=1)
    b, starts = vectors(A.shape[0])
    S = system(A, D.Jacobi(), reorder="rcm")
    for tag, x0 in starts:
        report("chip reordered jacobi %s chip_by_default=%d" % (tag, S.chip_info()["chip_by_default"]), S.solve(b, x0, max_iter=MAX_ITER))
    S.close()
    A = dirichlet(LAUNCH)
    b, starts = vectors(A.shape[0])
    x_true = torch.from_numpy(np.sin(np.arange(A.shape[0], dtype=np.float64))).cuda()
    for reorder in (None, "rcm"):
        S = system(A if reorder is None else O.unstructured_like(A, seed=1), D.Jacobi(), reorder=reorder)
        for flags, form in ((L.NO_SMALL, "graph replay"), (L.NO_SMALL | L.NO_GRAPH, "no graph")):
            for tag, x0 in starts:
                report("launch n=1600 jacobi %s %s reorder=%s" % (tag, form, reorder), S.solve(b, x0, max_iter=MAX_ITER, flags=flags))
        for tag, x0 in starts:
            res = S.solve(b, x0, max_iter=MAX_ITER, flags=L.NO_SMALL, x_true=x_true)
            report("launch n=1600 jacobi %s x_true reorder=%s" % (tag, reorder), res, " err=%s" % sha(np.asarray(res.err_history)))
        report("launch n=1600 jacobi x0=cos init_check_r reorder=%s" % reorder,
               S.solve(b, starts[1][1], max_iter=MAX_ITER, flags=L.NO_SMALL | L.INIT_CHECK_R))
        S.close()


def refined():
    A = dirichlet(LAUNCH)
    b, starts = vectors(A.shape[0])
    for kind, M, reorder in (("identity", D.Identity(), None), ("jacobi", D.Jacobi(), None), ("jacobi", D.Jacobi(), "rcm")):
        S = system(A if reorder is None else O.unstructured_like(A, seed=1), M, reorder=reorder)
        for tag, x0 in starts:
            res = S.solve_refined(b, x0, max_iter=MAX_ITER)
            report("refined n=1600 %s %s reorder=%s" % (kind, tag, reorder), res,
                   " outer_steps=%d outer=%s" % (res.outer_steps, sha(np.asarray(res.outer_history))))
        S.close()


def batches(reps):
    def run(name, mats, precond, flags=0, n_streams=4, time_it=False):
        systems = [system(A, precond(A)) for A in mats]
        rhs = [vectors(A.shape[0], seed=10 + i)[0] for i, A in enumerate(mats)]
        cos = [vectors(A.shape[0])[1][1][1] for A in mats]
        for tag, x0 in (("x0=None", None), ("x0=cos", cos)):
            out = solve_batch(systems, rhs, x0, max_iter=MAX_ITER, flags=flags, n_streams=n_streams)
            for i, res in enumerate(out):
                print("batch %s %s member=%d iterations=%d status=%d final_res=%s x=%s recurrence=%s" % (
                    name, tag, i, res.iterations, res.status, float(res.final_res).hex(), sha(res.x.detach().cpu().numpy()), res.recurrence),
                    flush=True)
        if time_it:
            timed("batch %s x0=None" % name, reps, lambda: solve_batch(systems, rhs, None, max_iter=MAX_ITER, flags=flags, n_streams=n_streams)[0].seconds)
        for S in systems:
            S.close()

    run("one_workgroup x8", [dirichlet((5 + i, 7)) for i in range(8)], lambda A: D.Jacobi(), time_it=True)
    run("team x9", [dirichlet(TEAM)] * 9, lambda A: D.Jacobi())
    run("chip x3", [O.poisson3d(41)] * 3, lambda A: D.Jacobi())
    run("ic0_solve x3 two streams", [dirichlet(LAUNCH)] * 3, lambda A: D.IC0("solve"), n_streams=2)
    run("single_reduction x2", [O.poisson3d(41)] * 2, lambda A: D.Jacobi(), flags=L.SINGLE_REDUCTION)
    run("one_workgroup x2 init_check_r", [dirichlet(SMALL)] * 2, lambda A: D.Jacobi(), flags=L.INIT_CHECK_R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    singles(args.reps)
    refined()
    batches(args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
