"""The single-reduction recurrence (DPCG_SINGLE_REDUCTION, include/dpcg.h; Chronopoulos and Gear, J. Comput. Appl. Math. 25, 1989)
restated in numpy, step by step.

Not a test.  `solve` runs the recurrence of dpcg_chip_sr.hip in its order: s = A z with the row sums in CSR order
(`oracle.c_oracle.spmv`), the three dot products of an update (four at k = 0), the test, then the scalars and the vector updates,
one product and one addition per entry.  Only the dot products have a free order, chosen by `tree`:

* `tree=None`: plain `np.dot` -- for the host tests, which ask what the recurrence computes, not in which bits;
* `tree={"rows_per_workgroup": per, ...}` (what `CsrSystem.chip_info()` reports; other keys are ignored): the whole-chip kernels'
  tree, restated from DESIGN section 4 -- workgroup w of 256 owns rows w * per .. (w + 1) * per, thread t of its 512 adds its rows
  w * per + t + 512 k in order, the 64 threads of a wave go through the wave tree, the 8 wave sums are added one after another,
  the 32 workgroup sums of a group go through the wave tree (lanes 32-63 hold +0.0), and so do the 8 group sums (lanes 8-63 hold
  +0.0).  With it history, count, status and x equal the device's bit for bit.
"""

from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from oracle import c_oracle as CO

OK, MAX_ITER, BREAKDOWN = 0, 1, 2
WORKGROUPS, THREADS = 256, 512


def wave_tree(v):
    """The 64-lane sum of the kernels' wave_sum over the last axis (a multiple of 64 is NOT split: exactly 64)."""
    assert v.shape[-1] == 64
    u = v.reshape(v.shape[:-1] + (4, 4, 4))
    q = (u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])                 # 4 rows x 4 quads
    row = (q[..., 3] + q[..., 2]) + (q[..., 1] + q[..., 0])
    return (row[..., 3] + row[..., 2]) + (row[..., 1] + row[..., 0])


def chip_dot(a, b, per):
    """<a,b> in the whole-chip kernels' tree; per = rows per workgroup (ceil(n / 256))."""
    n = a.shape[0]
    assert (n + WORKGROUPS - 1) // WORKGROUPS <= per and WORKGROUPS * per >= n
    rpt = (per + THREADS - 1) // THREADS
    prod = np.zeros(WORKGROUPS * per)
    prod[:n] = a * b                                                      # (rows that do not exist add +0.0: no bit changes)
    slots = np.zeros((WORKGROUPS, rpt * THREADS))
    slots[:, :per] = prod.reshape(WORKGROUPS, per)
    acc = np.zeros((WORKGROUPS, THREADS))
    for k in range(rpt):                                                  # a thread's rows in order
        acc = acc + slots[:, k * THREADS:(k + 1) * THREADS]
    waves = wave_tree(acc.reshape(WORKGROUPS, THREADS // 64, 64))         # [256][8]
    part = np.zeros(WORKGROUPS)
    for w in range(THREADS // 64):                                        # the 8 wave sums one after another
        part = part + waves[:, w]
    lanes = np.zeros((8, 64))
    lanes[:, :32] = part.reshape(8, 32)                                   # a group's 32 workgroup sums, lanes 32-63 hold +0.0
    top = np.zeros(64)
    top[:8] = wave_tree(lanes)                                            # the 8 group sums, lanes 8-63 hold +0.0
    return np.float64(wave_tree(top))


def solve(A, b, *, dinv=None, x0=None, rtol_sq=1e-8, atol_sq=0.0, max_iter=1024, init_check_r=False, tree=None):
    """M = I (dinv None) or Jacobi.  Returns a namespace: x, iterations, status (0 converged, 1 max_iter, 2 breakdown), res_history
    (iterations + 1 entries) and, per exchange, the sums gamma = <r,z>, delta = <z,Az>, rho (what the test of that exchange used)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    n = A.shape[0]
    b = np.ascontiguousarray(b, dtype=np.float64)
    if tree is None:
        dot = lambda u, v: np.float64(np.dot(u, v))
    else:
        per = int(tree["rows_per_workgroup"])
        dot = lambda u, v: chip_dot(u, v, per)
    apply_m = (lambda r: r.copy()) if dinv is None else (lambda r: np.asarray(dinv, dtype=np.float64) * r)
    if x0 is None:
        x, r = np.zeros(n), b.copy()
    else:
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        r = b - CO.spmv(A, x)
    z = apply_m(r)
    p, q = np.zeros(n), np.zeros(n)
    hist, gammas, deltas, rhos = [], [], [], []
    k, status = 0, MAX_ITER
    bb = gamma_prev = alpha_prev = np.float64(1.0)
    with np.errstate(all="ignore"):
        while True:
            s = CO.spmv(A, z)
            gamma, delta = dot(r, z), dot(z, s)
            rho = dot(z, z) if (k == 0 and not init_check_r) else dot(r, r)      # the reference's first test is on z
            if k == 0:
                bb = dot(b, b)
            gammas.append(gamma), deltas.append(delta), rhos.append(rho)
            res = rho / bb
            hist.append(res)
            if res < rtol_sq or rho < atol_sq:
                status = OK
                break
            if not res == res:
                status = BREAKDOWN
                break
            if k >= max_iter:
                break
            beta = np.float64(0.0) if k == 0 else gamma / gamma_prev
            den = delta if k == 0 else delta - (beta * gamma) / alpha_prev
            alpha = gamma / den
            gamma_prev, alpha_prev = gamma, alpha
            k += 1
            p = z + beta * p
            q = s + beta * q
            x = x + alpha * p
            r = r - alpha * q
            z = apply_m(r)
    return SimpleNamespace(x=x, iterations=k, status=status, res_history=np.array(hist), gamma=np.array(gammas),
                           delta=np.array(deltas), rho=np.array(rhos))
