"""The systems and cases of the mixed-precision PCG tests (test_refine_host.py, test_refine_gpu.py) and of tools/refine_probe.py."""

import functools

import numpy as np

import refine_restatement as R

MAX_ITER = 20000

SYSTEMS = {
    "poisson 5x7": lambda: R.poisson((5, 7)),                         # 35 rows: less than one workgroup, n % 4 = 3
    "poisson 33x31": lambda: R.poisson((33, 31)),                     # 1023 rows: odd, several workgroups, a tail
    "poisson 40x40": lambda: R.poisson((40, 40)),
    "shifted 32x32": lambda: R.shifted_laplacian((32, 32), 3),        # values that fp32 rounds
    "shifted 10x12x9": lambda: R.shifted_laplacian((10, 12, 9), 5),   # values that fp32 rounds
    "poisson 271x259": lambda: R.poisson((271, 259)),                 # 70 189 rows > kBlock * 64: the grid-stride loops turn over
}
CASES = [(name, pre, rtol_sq) for name in SYSTEMS for pre in ("identity", "jacobi") for rtol_sq in (1e-8, 1e-20)]


@functools.lru_cache(maxsize=None)
def system(name):
    """(A, b): b = default_rng(1).random(n)"""
    A = SYSTEMS[name]()
    return A, np.random.default_rng(1).random(A.shape[0])


@functools.lru_cache(maxsize=None)
def restated(name, pre, rtol_sq):
    """the restatement's solve of a case, computed once and shared (do not modify)"""
    A, b = system(name)
    return R.solve_refined(A, b, jacobi=pre == "jacobi", rtol_sq=rtol_sq, max_iter=MAX_ITER)
