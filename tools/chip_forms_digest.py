#!/usr/bin/env python3
"""Digest of one solve per whole-chip kernel family, for comparing two builds bit for bit (needs the GPU).

Every sum in the whole-chip kernels is added in a fixed order, so a solve is reproducible to the bit: a change that means to leave the
arithmetic alone must print the same lines before and after.  Per case, once with x0 = None and once with a non-zero x0: iteration
count, status, SHA-256 of res_history's bytes, SHA-256 of x's bytes -- and, with DPCG_CHIP_EVENTS=1, --reps N adds the kernel's time
between HIP events (min / median / max of N warmed solves) on a second line that starts with `#time`.

    python tools/chip_forms_digest.py [--reps N]            # the library to load: DPCG_LIBRARY, else the tree's own

The cases are the smallest systems the host path sends to each kernel: standard and single reduction with Jacobi, and standard with
M = I, on poisson3d(41); L L^T multiplied on poisson2d(79), 40 updates; resident triangular solves with IC(0) on poisson2d(40).  No
public call reaches the streamed triangular-solve kernel or an 8-rows-a-thread instantiation at a size that solves in seconds: no digest
covers them.  A tool, not a test: it pins nothing for a change that means to alter the arithmetic.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import deeppreconditioning_amd as D  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import oracle as O  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def chip_cases():
    """(name, matrix, preconditioner of a matrix, recurrence, max_iter) per whole-chip family (tools/solve_forms_digest.py takes them too)"""
    a3, a79, a40 = O.poisson3d(41), O.poisson2d(79), O.poisson2d(40)
    return [("standard_jacobi", a3, lambda A: D.Jacobi(), "standard", 1024),
            ("single_reduction_jacobi", a3, lambda A: D.Jacobi(), "single_reduction", 1024),
            ("standard_identity", a3, lambda A: D.Identity(), "standard", 1024),
            ("llt_multiply", a79, lambda A: D.LLtMultiply(CO.ic0(A)), "standard", 40),
            ("triangular_solves_resident", a40, lambda A: D.IC0("solve", ordering="multicolor"), "standard", 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=0)
    args = ap.parse_args()
    for name, A, precond, recurrence, max_iter in chip_cases():
        n = A.shape[0]
        b = torch.from_numpy(np.ascontiguousarray(O.rhs(n, 0))).cuda()
        x0 = torch.from_numpy(np.ascontiguousarray(np.cos(np.arange(n, dtype=np.float64)))).cuda()
        S = D.CsrSystem.from_any(A, reorder=None)
        S.set_preconditioner(precond(A))
        assert S.chip_info()["chip_by_default"], (name, S.chip_info())
        for tag, start in (("x0=None", None), ("x0=cos", x0)):
            res = S.solve(b, start, recurrence=recurrence, max_iter=max_iter)
            assert S.chip_info()["chip_by_default"], (name, S.chip_info())
            x = res.x.detach().cpu().numpy()
            print("%s %s iterations=%d status=%d hist=%s x=%s" % (name, tag, res.iterations, res.status, sha(np.asarray(res.res_history)), sha(x)), flush=True)
            if args.reps > 0:
                for _ in range(3):
                    S.solve(b, start, recurrence=recurrence, max_iter=max_iter)
                ms = []
                for _ in range(args.reps):
                    S.solve(b, start, recurrence=recurrence, max_iter=max_iter)
                    ms.append(S.chip_info()["kernel_ms"])
                print("#time %s %s kernel_ms min=%.4f median=%.4f max=%.4f reps=%d" % (name, tag, min(ms), float(np.median(ms)), max(ms), args.reps), flush=True)
        S.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
