#!/usr/bin/env python3
"""Digest of the null-space and the deflated solves (dpcg_projected.h) and of the plain launch path, for comparing two builds bit
for bit (needs the GPU).

Every sum in these kernels is added in a fixed order, so a solve is reproducible to the bit: a change that means to leave the
arithmetic alone must print the same lines before and after.  Per case: iteration count, status, SHA-256 of res_history's bytes,
SHA-256 of x's bytes.

    python tools/projected_forms_digest.py            # the library to load: DPCG_LIBRARY, else the tree's own

Cases (every solve at most 200 updates; a case that stops at the cap is as good a digest as one that converges):
  null space   the constant column and k = 1, 2, 3, 4 stored columns (the ones vector plus indicators of disconnected Neumann blocks,
               as tests/test_nullspace_gpu.py builds them)
  deflation    k = 1, 2, 3 (stored as 4), 5 (stored as 8), 8 columns: indicators of k contiguous runs of the rows
  each with    M = I, Jacobi, IC(0) multiplied -- of A + 0.05 I where A is singular -- (the vector kernels' three forms);  n = 35 (5 x 7: odd, one workgroup), 1 023
               (33 x 31: odd, four workgroups), 1 600 (40 x 40);  x0 = None and x0 = cos(i)
  call forms   DPCG_INIT_CHECK_R and a reordered handle, once per family
  plain path   the definite 40 x 40 system, Jacobi, DPCG_NO_SMALL: by graph replay and with DPCG_NO_GRAPH
A tool, not a test: it pins nothing for a change that means to alter the arithmetic.  One process, no retries.
"""
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import deeppreconditioning_amd as D  # noqa: E402
from deeppreconditioning_amd import _lib as L  # noqa: E402
from deeppreconditioning_amd.poisson import neumann_csr  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402

GRIDS = [(5, 7), (33, 31), (40, 40)]
MAX_ITER = 200


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def csr32(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    A.indices, A.indptr = A.indices.astype(np.int32), A.indptr.astype(np.int32)
    return A


def bands(rows, k):
    """rows cut into k runs as evenly as they go, the larger ones first"""
    return [rows // k + (1 if i < rows % k else 0) for i in range(k)]


def neumann_blocks(grid, k):
    """The pure-Neumann Laplacian of k disconnected row bands of the grid (seeded weights), and [1_all, 1_band1, ...]: its null space,
    neither normalised nor orthogonal."""
    rows, width = grid
    parts = bands(rows, k)
    A = csr32(sp.block_diag([neumann_csr((r, width), 3) for r in parts], format="csr"))
    Z = np.zeros((A.shape[0], k))
    Z[:, 0] = 1.0
    at = 0
    for j, r in enumerate(parts[:-1]):
        Z[at:at + r * width, j + 1] = 1.0
        at += r * width
    return A, Z


def dirichlet(grid):
    A = None
    for d in grid:
        T = sp.diags([-np.ones(d - 1), 2.0 * np.ones(d), -np.ones(d - 1)], [-1, 0, 1], format="csr")
        A = T if A is None else sp.kron(sp.identity(T.shape[0]), A) + sp.kron(T, sp.identity(A.shape[0]))
    return csr32(A)


def chunk_indicators(n, k):
    """k columns, column j = 1 on the j-th of k contiguous runs of the n rows"""
    edges = np.concatenate([[0], np.cumsum(bands(n, k))])
    W = np.zeros((n, k))
    for j in range(k):
        W[edges[j]:edges[j + 1], j] = 1.0
    return W


def precond(kind, A, shift=0.0):
    """ic0_multiply: z = L (L^T r) with the IC(0) factor of A + shift I (IC(0) of a singular A breaks down at its last pivot)"""
    if kind == "ic0_multiply":
        return D.LLtMultiply(CO.ic0(csr32(A + shift * sp.identity(A.shape[0], format="csr"))))
    return D.Jacobi() if kind == "jacobi" else None


def report(name, S, b, x0, **kw):
    res = S.solve(b, x0, max_iter=MAX_ITER, **kw)
    print("%s iterations=%d status=%d hist=%s x=%s" % (name, res.iterations, res.status, sha(np.asarray(res.res_history)),
                                                      sha(res.x.detach().cpu().numpy())), flush=True)


def main():
    torch.cuda.set_device(0)
    for grid in GRIDS:
        n = grid[0] * grid[1]
        b = torch.from_numpy(np.random.default_rng(1).random(n)).cuda()
        x0 = torch.from_numpy(np.cos(np.arange(n, dtype=np.float64))).cuda()
        starts = (("x0=None", None), ("x0=cos", x0))
        for shape in ("constant", 1, 2, 3, 4):
            A, Z = neumann_blocks(grid, 1 if shape == "constant" else shape)
            for kind in ("identity", "jacobi", "ic0_multiply"):
                S = D.CsrSystem.from_any(A, reorder=None)
                S.set_preconditioner(precond(kind, A, 0.05))
                S.set_nullspace("constant" if shape == "constant" else Z)
                for tag, start in starts:
                    report("nullspace n=%d Z=%s %s %s" % (n, shape, kind, tag), S, b, start)
                S.close()
        A = dirichlet(grid)
        for k in (1, 2, 3, 5, 8):
            for kind in ("identity", "jacobi", "ic0_multiply"):
                S = D.CsrSystem.from_any(A, reorder=None)
                S.set_preconditioner(precond(kind, A))
                S.set_deflation(chunk_indicators(n, k))
                for tag, start in starts:
                    report("deflation n=%d k=%d %s %s" % (n, k, kind, tag), S, b, start)
                S.close()
    # the call forms, on 33 x 31
    grid = GRIDS[1]
    n = grid[0] * grid[1]
    b = torch.from_numpy(np.random.default_rng(1).random(n)).cuda()
    x0 = torch.from_numpy(np.cos(np.arange(n, dtype=np.float64))).cuda()
    A2, Z2 = neumann_blocks(grid, 2)
    Ad, Wd = dirichlet(grid), chunk_indicators(n, 3)
    for reorder, flags, tag in ((None, L.INIT_CHECK_R, "init_check_r"), ("rcm", 0, "reordered")):
        S = D.CsrSystem.from_any(A2, reorder=reorder)
        S.set_preconditioner(D.Jacobi())
        S.set_nullspace(Z2)
        assert (reorder is None) or S.reordered
        report("nullspace n=%d Z=2 jacobi x0=cos %s" % (n, tag), S, b, x0, flags=flags)
        S.close()
        S = D.CsrSystem.from_any(Ad, reorder=reorder)
        S.set_preconditioner(D.Jacobi())
        S.set_deflation(Wd)
        assert (reorder is None) or S.reordered
        report("deflation n=%d k=3 jacobi x0=cos %s" % (n, tag), S, b, x0, flags=flags)
        S.close()
    # the plain launch path: its driver shares the staging, the wait and the delivery
    grid = GRIDS[2]
    n = grid[0] * grid[1]
    b = torch.from_numpy(np.random.default_rng(1).random(n)).cuda()
    x0 = torch.from_numpy(np.cos(np.arange(n, dtype=np.float64))).cuda()
    S = D.CsrSystem.from_any(dirichlet(grid), reorder=None)
    S.set_preconditioner(D.Jacobi())
    for flags, tag in ((L.NO_SMALL, "graph replay"), (L.NO_SMALL | L.NO_GRAPH, "no graph")):
        for stag, start in (("x0=None", None), ("x0=cos", x0)):
            report("plain n=%d jacobi %s %s" % (n, stag, tag), S, b, start, flags=flags)
    S.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
