"""The projected initial guess (dpcg_guess_*, include/dpcg.h; Fischer, CMAME 163, 1998) restated in numpy, step by step.

Not a test.  `Guess` keeps an A-orthonormal basis X~ (columns) and W = A X~ exactly as the device object does and makes the same
decisions in the same order; only the long sums (dot products over the rows) have a free order, chosen by `sums`:
"sequential" (first row to last) or "pairwise" (numpy's blocked pairwise sum) -- two legitimate orders whose distance is the
yardstick of tests/test_guess_gpu.py.  Linear combinations run over the columns in ascending order, one product and one
addition per column, as the kernels do; the small host-side steps (Cholesky of the Gram matrix, R^-1, the dependence test) are
loops in the order of dpcg_guess.hip.
"""

import numpy as np
import scipy.sparse as sp


def _dot(a, b, sums):
    p = a * b
    if p.size == 0:
        return 0.0
    return float(np.cumsum(p)[-1]) if sums == "sequential" else float(np.sum(p))


def _combine(X, c):
    """sum_i c_i X[:, i], columns ascending, starting from zero."""
    acc = np.zeros(X.shape[0])
    for i in range(len(c)):
        acc = acc + c[i] * X[:, i]
    return acc


class Guess:
    def __init__(self, A, depth=8, tol_dep=1e-7, sums="sequential"):
        if not 1 <= depth <= 32:
            raise ValueError("depth must lie in 1 .. 32")
        if not tol_dep > 0:
            raise ValueError("tol_dep must be positive")
        assert sums in ("sequential", "pairwise")
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.n = self.A.shape[0]
        self.depth, self.tol_dep, self.sums = depth, tol_dep, sums
        self.X = np.zeros((self.n, 0))
        self.W = np.zeros((self.n, 0))
        self.x0 = np.zeros(self.n)
        self.c = np.zeros(0)
        self.c_valid = False            # x0 = X~ c holds for the basis as it stands
        self.stale = False              # the matrix changed since the basis was last made consistent
        self.epoch = 0
        self.counters = dict(restarts=0, appended=0, skipped=0, dropped=0, reorthonormalisations=0)

    # -- bookkeeping ---------------------------------------------------------------------------------------------------------
    @property
    def size(self):
        return self.X.shape[1]

    def info(self):
        return dict(depth=self.depth, size=self.size, values_epoch=self.epoch, **self.counters)

    def basis(self):
        return self.X.copy(), self.W.copy()

    def reset(self):
        self.X = np.zeros((self.n, 0))
        self.W = np.zeros((self.n, 0))
        self.c_valid = False
        for k in self.counters:
            self.counters[k] = 0

    def set_matrix(self, A):
        """dpcg_update_values: new values; the basis is made consistent before its next use."""
        self.A = sp.csr_matrix(A, dtype=np.float64)
        self.stale = True
        self.epoch += 1

    def _dots(self, X, v):
        return np.array([_dot(X[:, i], v, self.sums) for i in range(X.shape[1])])

    # -- the matrix changed: W = A X~, then CholQR2 ------------------------------------------------------------------------------
    def _reorthonormalise(self):
        l = self.size
        X = self.X
        W = np.column_stack([self.A @ X[:, j] for j in range(l)]) if l else np.zeros((self.n, 0))
        tol2 = self.tol_dep * self.tol_dep
        for _ in range(2):
            if l == 0:
                break
            G = np.zeros((l, l))
            for j in range(l):
                G[:, j] = self._dots(X, W[:, j])
            R = np.zeros((l, l))
            keep = l
            for j in range(l):                      # G = R^T R from the upper triangle, sums over k ascending
                p = G[j, j]
                for k in range(j):
                    p = p - R[k, j] * R[k, j]
                if not np.isfinite(p) or not p > tol2 * G[j, j]:
                    keep = j
                    break
                R[j, j] = np.sqrt(p)
                for m in range(j + 1, l):
                    t = G[j, m]
                    for k in range(j):
                        t = t - R[k, j] * R[k, m]
                    R[j, m] = t / R[j, j]
            self.counters["dropped"] += l - keep
            T = np.zeros((keep, keep))
            for j in range(keep):                   # T = R^-1, column by column
                T[j, j] = 1.0 / R[j, j]
                for i in range(j - 1, -1, -1):
                    t = 0.0
                    for k in range(i + 1, j + 1):
                        t = t + R[i, k] * T[k, j]
                    T[i, j] = -t / R[i, i]
            l = keep
            if l == 0:
                break
            Xn, Wn = np.zeros((self.n, l)), np.zeros((self.n, l))
            for j in range(l):                      # B <- B T: column j = sum_{i <= j} B[:, i] T[i, j], i ascending
                Xn[:, j] = _combine(X[:, : j + 1], T[: j + 1, j])
                Wn[:, j] = _combine(W[:, : j + 1], T[: j + 1, j])
            X, W = Xn, Wn
        self.X, self.W = X[:, :l], W[:, :l]
        self.counters["reorthonormalisations"] += 1
        self.stale = False
        self.c_valid = False

    # -- project / update -------------------------------------------------------------------------------------------------
    def project(self, b):
        b = np.asarray(b, dtype=np.float64)
        if b.shape != (self.n,):
            raise ValueError("wrong length")
        if self.stale:
            self._reorthonormalise()
        if not np.all(np.isfinite(b)):
            raise ValueError("non-finite b")
        c = self._dots(self.X, b)
        self.x0 = _combine(self.X, c)
        self.c = c
        self.c_valid = True
        return self.x0.copy()

    def update(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.n,):
            raise ValueError("wrong length")
        if self.stale:
            self._reorthonormalise()
        if not np.all(np.isfinite(x)):
            raise ValueError("non-finite x")
        restart = self.size == self.depth
        l = 0 if restart else self.size
        use_x0 = not restart and self.c_valid
        X, W = self.X[:, :l], self.W[:, :l]
        d = x - self.x0 if use_x0 else x.copy()
        w = self.A @ d
        g_sum = np.zeros(l)
        if use_x0:
            g_sum[: len(self.c)] = self.c[:l]
        for _ in range(2 if l else 0):              # classical Gram-Schmidt twice in the A inner product
            g = self._dots(X, w)
            d = d - _combine(X, g)
            w = w - _combine(W, g)
            g_sum = g_sum + g
        s = _dot(d, w, self.sums)
        in_span = 0.0
        for e in g_sum:
            in_span = in_span + e * e
        xax = in_span + s                           # <x, A x>: x = X~ (c + g) + d
        if not np.isfinite(s) or not s > self.tol_dep * self.tol_dep * xax:
            self.counters["skipped"] += 1
            return
        root = np.sqrt(s)
        if restart:
            self.X, self.W = np.zeros((self.n, 0)), np.zeros((self.n, 0))
            self.counters["restarts"] += 1
            self.c_valid = False
        else:
            self.counters["appended"] += 1
            self.c = np.concatenate([self.c[:l], np.zeros(1)]) if use_x0 else self.c
        self.X = np.column_stack([self.X, d / root])
        self.W = np.column_stack([self.W, w / root])


def xax_direct(A, x):
    """<x, A x> as the issue states it -- what Guess.update's |c + g|^2 + s equals up to rounding."""
    return float(x @ (A @ x))
