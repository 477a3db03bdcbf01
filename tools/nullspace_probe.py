"""us per update of the null-space driver (dpcg_nullspace.hip) against the multi-launch path of a definite solve.

    python tools/nullspace_probe.py            # writes profiles/nullspace_probe.md

Systems: the pure-Neumann Laplacian of a 128 x 128 and of a 100 x 100 x 100 box (unit weights).  Null-space runs: "constant"
(Z never read), an explicit ones vector (general kernels, k = 1), and k = 2 on the same number of rows cut into two closed
halves (128 x 64 twice, 100 x 100 x 50 twice: one interface of edges fewer).  Baseline: the same box matrix with one row pinned
(a_00 += 1: definite), no null space, DPCG_NO_SMALL | DPCG_NO_TEAM -- the multi-launch path, which this feature does not touch
(a handle without a null space runs the code it ran before) -- as it runs by default there (two-kernel updates and replayed graphs
where the driver chooses them) and as three plain launches per update (+ DPCG_NO_FUSE | DPCG_NO_GRAPH), the form the null-space
driver has.  Every run does exactly UPDATES updates (rtol_sq = 0 never passes); the time is the driver's own loop time, the best
of REPEATS runs after one warm-up.
"""

import pathlib
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import deeppreconditioning_amd as D  # noqa: E402
from deeppreconditioning_amd import _lib as L  # noqa: E402
from deeppreconditioning_amd.poisson import neumann_csr  # noqa: E402

UPDATES, REPEATS = 300, 5


def us_per_update(S, b, flags=0):
    best = np.inf
    for rep in range(REPEATS + 1):
        res = S.solve(b, rtol_sq=0.0, max_iter=UPDATES, flags=flags, want_history=False)
        assert res.iterations == UPDATES and res.status == L.MAX_ITER, (res.iterations, res.status)
        if rep > 0:
            best = min(best, res.seconds / UPDATES * 1e6)
    return best


def halves(dims):
    half = tuple(dims[:-1]) + (dims[-1] // 2,)
    A = sp.csr_matrix(sp.block_diag([neumann_csr(half), neumann_csr(half)], format="csr"))
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    n = A.shape[0]
    Z = np.zeros((n, 2))
    Z[:, 0] = 1.0
    Z[: n // 2, 1] = 1.0
    return A, Z


def main():
    torch.cuda.set_device(0)
    rows = []
    for dims in ((128, 128), (100, 100, 100)):
        A = neumann_csr(dims)
        n = A.shape[0]
        b = torch.from_numpy(np.random.default_rng(1).random(n)).cuda()
        pinned = A.copy()
        pinned.data[pinned.indptr[0] + int(np.flatnonzero(pinned.indices[pinned.indptr[0]:pinned.indptr[1]] == 0)[0])] += 1.0
        A2, Z2 = halves(dims)
        for pre_name, pre in (("Identity", None), ("Jacobi", D.Jacobi)):
            out = {}
            Sb = D.CsrSystem.from_any(pinned, reorder=None)
            Sb.set_preconditioner(pre() if pre else None)
            out["baseline"] = us_per_update(Sb, b, L.NO_SMALL | L.NO_TEAM)
            out["baseline, 3 plain launches"] = us_per_update(Sb, b, L.NO_SMALL | L.NO_TEAM | L.NO_FUSE | L.NO_GRAPH)
            for label, M, ns in (("constant k=1", A, "constant"), ("general k=1", A, np.ones(n)), ("general k=2", A2, Z2)):
                S = D.CsrSystem.from_any(M, reorder=None)
                S.set_preconditioner(pre() if pre else None)
                S.set_nullspace(ns)
                out[label] = us_per_update(S, b)
            rows.append(("x".join(map(str, dims)), n, pre_name, out))
            print(rows[-1], flush=True)
    cols = ["baseline", "baseline, 3 plain launches", "constant k=1", "general k=1", "general k=2"]
    name = torch.cuda.get_device_properties(0).gcnArchName
    lines = ["# Null-space PCG: us per update", "",
             f"`python tools/nullspace_probe.py` on {name}: {UPDATES} updates per run, best of {REPEATS} after a warm-up, the driver's loop time.",
             "Baseline: the box matrix with one row pinned (definite), no null space, `DPCG_NO_SMALL | DPCG_NO_TEAM` -- the multi-launch",
             "path of a definite solve, which the feature leaves as it was -- by default and as three plain launches per update",
             "(`+ DPCG_NO_FUSE | DPCG_NO_GRAPH`), the form the null-space driver has.  k = 2 runs on the same rows cut into two closed halves.", "",
             "| system | rows | M | " + " | ".join(cols) + " |", "|---|---|---|" + "---|" * len(cols)]
    for dims, n, pre_name, out in rows:
        lines.append(f"| {dims} | {n} | {pre_name} | " + " | ".join(f"{out[c]:.2f}" for c in cols) + " |")
    path = ROOT / "profiles" / "nullspace_probe.md"
    path.parent.mkdir(exist_ok=True)
    path.write_text("\n".join(lines) + "\n")
    print(path.read_text())


if __name__ == "__main__":
    main()
