// Projected initial guess for a sequence of systems on one handle (dpcg_guess_*, include/dpcg.h): P. F. Fischer, "Projection
// techniques for iterative solution of Ax = b with successive right-hand sides", CMAME 163 (1998).  Not in the reference -- its
// callers start every solve from zeros (cg.py:58).
//
// State.  A basis X~ = [x~_0 .. x~_{l-1}], l <= depth, with x~_i^T A x~_j = delta_ij, and W = A X~, both in the CALLER's numbering.
//   project(b):  c = X~^T b;  x0 = X~ c  -- the A-norm-best approximation of A^-1 b in the span (l = 0: zeros).
//   update(x):   d = x - x0;  w = A d (the handle's SpMV);  classical Gram-Schmidt twice in the A inner product,
//                g = X~^T w, d -= X~ g, w -= W g (no second SpMV);  s = <d, w>;  the direction is dependent, and not appended, when
//                s <= tol_dep^2 <x, A x> or s is not finite;  otherwise x~_l = d / sqrt(s), W_l = w / sqrt(s).
//                <x, A x> costs nothing: x = X~ (c + g) + d with g the sum of both passes' coefficients, so it is |c + g|^2 + s.
//                A full basis (l == depth) restarts instead: x0 is left out (d = x), nothing is projected out, and the basis
//                becomes the one vector x / ||x||_A.  The x0 of the last project is used only while the basis it came from stands
//                (no restart, re-orthonormalisation or reset since); otherwise d = x.
//   new values:  (the handle's values epoch moved)  W = A X~ by l SpMVs; twice (CholQR2): G = X~^T W on the device, G = R^T R on
//                the host, direction j and all later ones dropped at the first pivot <= tol_dep^2 G_jj, X~ <- X~ R^-1, W <- W R^-1.
//
// Layout (as dpcg_lanczos.hip's basis).  X~ and W are column-major, the column length padded to a multiple of 1024 rows (ld),
// the padding rows zero: the kernels run over ld rows without bounds tests on the basis.  A lane owns 2 consecutive rows (one
// 16-byte load per column) at every size.  The caller's vectors have n rows and any alignment: they are read and written
// 16 bytes at a time where their address allows it, row by row otherwise and in the last, partial group.
//
// Kernels, each one pass over its l columns (l n 8 bytes; k_gs_pair reads X~ and W: twice that):
//   k_gs_dots      per-wave partials of X^T v for columns 0 .. l-1 (and of sum 0 v_i: NaN exactly when v holds a non-finite value)
//   k_gs_fin       column i's partials summed in one fixed order (workgroup i)
//   k_gs_combine   y = X c  |  y = v - X c
//   k_gs_pair      d -= X g, w -= W g, optionally the partials of <d, w>
//   k_gs_rmul      X <- X R^-1 and W <- W R^-1 in place: a lane holds its rows' l values in registers, R^-1 sits in LDS
//   k_gs_append    x~_l = d / sqrt(s), W_l = w / sqrt(s)
// No float atomics: every sum has one order, two runs give the same bits.  project and update read a few scalars back and so
// synchronise the stream once per call.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"

struct dpcg_guess {
    dpcg_system *h = nullptr;        // null once the system has been destroyed: every call is then DPCG_ERR_STATE
    int depth = 0, size = 0;
    double tol_dep = 0.0;
    int64_t n = 0, ld = 0, nw = 0;   // nw: waves of a vector kernel = partials per column
    double *X = nullptr, *W = nullptr;                  // depth x ld each
    double *x0 = nullptr, *d = nullptr, *w = nullptr;   // ld each, padding rows zero
    double *part = nullptr;          // (depth + 1) x nw
    double *coef = nullptr;          // device scalars (kCoef* below)
    bool c_valid = false;            // x0 = X~ c_host holds for the basis as it stands
    double c_host[32];
    uint64_t epoch = 0;              // the handle's values epoch the basis is consistent with
    int restarts = 0, appended = 0, skipped = 0, dropped = 0, reorthos = 0;
    std::vector<double> rinv_host;
};

namespace dpcg {
namespace {

constexpr int kGsMaxDepth = 32;
constexpr int kGsSpan = 1024;                 // ld is a multiple of it
constexpr int kGsRows = 2;                    // consecutive rows a lane owns: one 16-byte load per column
// coef, the device scalars: the coefficients of the first Gram-Schmidt pass (project: c and, behind it, the probe of b: depth + 1
// slots), those of the second pass, s = <d, w>, the probe of x -- update reads [0, kCoefRead) back in one copy --, the constant 1, the
// Gram matrix and R^-1
constexpr int kCoefG1 = 0, kCoefG2 = kCoefG1 + kGsMaxDepth + 1, kCoefS = kCoefG2 + kGsMaxDepth, kCoefProbe = kCoefS + 1,
              kCoefRead = kCoefProbe + 1, kCoefOne = kCoefRead, kCoefGram = kCoefOne + 1,
              kCoefRinv = kCoefGram + kGsMaxDepth * kGsMaxDepth, kCoefCount = kCoefRinv + kGsMaxDepth * kGsMaxDepth;
static_assert(kCoefG2 >= kCoefG1 + kGsMaxDepth + 1 && kCoefS >= kCoefG2 + kGsMaxDepth && kCoefRead > kCoefProbe && kCoefRead > kCoefS,
              "the blocks of the scalar buffer overlap, or update's read-back misses one");
enum GsUser { GS_PADDED = 0, GS_USER_VEC = 1, GS_USER_SCALAR = 2 };   // whose vector: ours (ld rows), the caller's (n rows)

template <int ROWS>
__device__ __forceinline__ void gs_load(const double *p, double (&v)[ROWS]) {
#pragma unroll
    for (int h = 0; h < ROWS / 2; ++h) {
        const double2 q = reinterpret_cast<const double2 *>(p)[h];
        v[2 * h] = q.x;
        v[2 * h + 1] = q.y;
    }
}
template <int ROWS>
__device__ __forceinline__ void gs_store(double *p, const double (&v)[ROWS]) {
#pragma unroll
    for (int h = 0; h < ROWS / 2; ++h) reinterpret_cast<double2 *>(p)[h] = make_double2(v[2 * h], v[2 * h + 1]);
}
// rows row .. row + ROWS - 1 of a vector that may be the caller's: n rows, rows beyond read as zero
template <int ROWS>
__device__ __forceinline__ void gs_load_any(const double *v, int kind, int64_t row, int64_t n, double (&x)[ROWS]) {
    if (kind == GS_PADDED || (kind == GS_USER_VEC && row + ROWS <= n)) {
        gs_load<ROWS>(v + row, x);
    } else {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) x[k] = row + k < n ? v[row + k] : 0.0;
    }
}
template <int ROWS>
__device__ __forceinline__ void gs_store_user(double *v, int kind, int64_t row, int64_t n, const double (&x)[ROWS]) {
    if (kind == GS_USER_VEC && row + ROWS <= n) {
        gs_store<ROWS>(v + row, x);
    } else {
#pragma unroll
        for (int k = 0; k < ROWS; ++k)
            if (row + k < n) v[row + k] = x[k];
    }
}

// part[i * nw + wave] = <X[:, i], v> over the wave's 64 ROWS rows, i < l; probe: part[l * nw + wave] = sum 0 * v_i.
// Grid: ld / (kBlock ROWS) workgroups, exact.
template <int ROWS>
__global__ __launch_bounds__(kBlock) void k_gs_dots(int64_t ld, int64_t n, int l, const double *__restrict__ X,
                                                    const double *__restrict__ v, int v_kind, int probe, double *__restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t row = t * ROWS;
    const int64_t nw = ld / (64 * ROWS);
    const int64_t wave = t >> 6;
    const bool writer = (threadIdx.x & 63) == 63;
    double x[ROWS];
    gs_load_any<ROWS>(v, v_kind, row, n, x);
    constexpr int U = 4;      // columns whose loads are in flight before their reductions
    int i = 0;
    for (; i + U <= l; i += U) {
        double s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double z[ROWS];
            gs_load<ROWS>(X + (int64_t)(i + u) * ld + row, z);
            s[u] = 0.0;
#pragma unroll
            for (int k = 0; k < ROWS; ++k) s[u] = s[u] + z[k] * x[k];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double r = wave_sum(s[u]);
            if (writer) part[(int64_t)(i + u) * nw + wave] = r;
        }
    }
    for (; i < l; ++i) {
        double z[ROWS];
        gs_load<ROWS>(X + (int64_t)i * ld + row, z);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) s = s + z[k] * x[k];
        const double r = wave_sum(s);
        if (writer) part[(int64_t)i * nw + wave] = r;
    }
    if (probe) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) s = s + 0.0 * x[k];
        const double r = wave_sum(s);
        if (writer) part[(int64_t)l * nw + wave] = r;
    }
}

// out[i] = sum over the nw partials of column i, in one fixed order (workgroup i)
__global__ __launch_bounds__(kBlock) void k_gs_fin(const double *__restrict__ part, int64_t nw, double *__restrict__ out) {
    __shared__ double sh[4];
    const double *p = part + (int64_t)blockIdx.x * nw;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < nw; k += kBlock) s += p[k];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// MODE 0: y = X c.  MODE 1: y = v - X c, and part[wave] = sum 0 * v_i (the probe of v).  X c is summed over the columns in
// ascending order.  y: ours (ld rows; the padding rows come out zero); y_user (may be null): the caller's copy of it, n rows.
template <int MODE, int ROWS>
__global__ __launch_bounds__(kBlock) void k_gs_combine(int64_t ld, int64_t n, int l, const double *__restrict__ X,
                                                       const double *__restrict__ c, const double *__restrict__ v, int v_kind,
                                                       double *__restrict__ y, double *__restrict__ y_user, int y_kind,
                                                       double *__restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t row = t * ROWS;
    double acc[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) acc[k] = 0.0;
#pragma unroll 8
    for (int i = 0; i < l; ++i) {
        const double ci = c[i];
        double z[ROWS];
        gs_load<ROWS>(X + (int64_t)i * ld + row, z);
#pragma unroll
        for (int k = 0; k < ROWS; ++k) acc[k] = acc[k] + ci * z[k];
    }
    if (MODE == 1) {
        double x[ROWS];
        gs_load_any<ROWS>(v, v_kind, row, n, x);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            s = s + 0.0 * x[k];
            acc[k] = x[k] - acc[k];
        }
        const double r = wave_sum(s);
        if ((threadIdx.x & 63) == 63) part[t >> 6] = r;
    }
    gs_store<ROWS>(y + row, acc);
    if (y_user) gs_store_user<ROWS>(y_user, y_kind, row, n, acc);
}

// d -= X g, w -= W g (columns ascending); part (may be null): part[wave] = <d, w> of the new vectors
template <int ROWS>
__global__ __launch_bounds__(kBlock) void k_gs_pair(int64_t ld, int l, const double *__restrict__ X, const double *__restrict__ W,
                                                    const double *__restrict__ g, double *__restrict__ d, double *__restrict__ w,
                                                    double *__restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t row = t * ROWS;
    double ad[ROWS], aw[ROWS], dv[ROWS], wv[ROWS];
    gs_load<ROWS>(d + row, dv);
    gs_load<ROWS>(w + row, wv);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) ad[k] = aw[k] = 0.0;
#pragma unroll 4
    for (int i = 0; i < l; ++i) {
        const double gi = g[i];
        double zx[ROWS], zw[ROWS];
        gs_load<ROWS>(X + (int64_t)i * ld + row, zx);
        gs_load<ROWS>(W + (int64_t)i * ld + row, zw);
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            ad[k] = ad[k] + gi * zx[k];
            aw[k] = aw[k] + gi * zw[k];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        dv[k] = dv[k] - ad[k];
        wv[k] = wv[k] - aw[k];
        s = s + dv[k] * wv[k];
    }
    if (l > 0) {
        gs_store<ROWS>(d + row, dv);
        gs_store<ROWS>(w + row, wv);
    }
    if (part) {
        const double r = wave_sum(s);
        if ((threadIdx.x & 63) == 63) part[t >> 6] = r;
    }
}

// column = d / sqrt(s) and w / sqrt(s) over ld rows (the padding rows of d and w are zero)
template <int ROWS>
__global__ __launch_bounds__(kBlock) void k_gs_append(const double *__restrict__ d, const double *__restrict__ w,
                                                      double *__restrict__ x_col, double *__restrict__ w_col, double root) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * ROWS;
    double a[ROWS], b[ROWS];
    gs_load<ROWS>(d + row, a);
    gs_load<ROWS>(w + row, b);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        a[k] = a[k] / root;
        b[k] = b[k] / root;
    }
    gs_store<ROWS>(x_col + row, a);
    gs_store<ROWS>(w_col + row, b);
}

// B <- B T in place for B = X (blockIdx.y = 0) and B = W (1), T = rinv (l x l, row-major, upper triangular): column j of the
// result is sum_{i <= j} B[:, i] T[i][j], i ascending.  A lane owns 2 rows and holds their l values in registers (LMAX >= l:
// 8, 16 or 32 -- up to 128 VGPRs); T is staged in LDS (every lane reads the same word: a broadcast).  Grid: (ld / 512, 2).
template <int LMAX>
__global__ __launch_bounds__(kBlock) void k_gs_rmul(int64_t ld, int l, double *__restrict__ X, double *__restrict__ W,
                                                    const double *__restrict__ rinv) {
    __shared__ double T[LMAX * LMAX];
    for (int k = threadIdx.x; k < l * l; k += kBlock) T[(k / l) * LMAX + k % l] = rinv[k];
    __syncthreads();
    double *B = blockIdx.y == 0 ? X : W;
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
    double a0[LMAX], a1[LMAX];
#pragma unroll
    for (int i = 0; i < LMAX; ++i) {
        a0[i] = a1[i] = 0.0;
        if (i < l) {
            const double2 q = *reinterpret_cast<const double2 *>(B + (int64_t)i * ld + row);
            a0[i] = q.x;
            a1[i] = q.y;
        }
    }
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        if (j < l) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int i = 0; i <= j; ++i) {
                const double tij = T[i * LMAX + j];
                s0 = s0 + a0[i] * tij;
                s1 = s1 + a1[i] * tij;
            }
            *reinterpret_cast<double2 *>(B + (int64_t)j * ld + row) = make_double2(s0, s1);
        }
    }
}

inline int user_kind(const void *p) { return (((uintptr_t)p) & 15) == 0 ? GS_USER_VEC : GS_USER_SCALAR; }

void launch_dots(const dpcg_guess *g, int l, const double *X, const double *v, int v_kind, bool probe, double *out, hipStream_t s) {
    const int grid = (int)(g->ld / (kBlock * kGsRows));
    hipLaunchKernelGGL((k_gs_dots<kGsRows>), dim3(grid), dim3(kBlock), 0, s, g->ld, g->n, l, X, v, v_kind, probe ? 1 : 0, g->part);
    const int cols = l + (probe ? 1 : 0);
    if (cols > 0) hipLaunchKernelGGL(k_gs_fin, dim3(cols), dim3(kBlock), 0, s, g->part, g->nw, out);
}

template <int MODE>
void launch_combine(const dpcg_guess *g, int l, const double *X, const double *c, const double *v, int v_kind, double *y,
                    double *y_user, hipStream_t s) {
    const int grid = (int)(g->ld / (kBlock * kGsRows));
    const int y_kind = y_user ? user_kind(y_user) : GS_PADDED;
    hipLaunchKernelGGL((k_gs_combine<MODE, kGsRows>), dim3(grid), dim3(kBlock), 0, s, g->ld, g->n, l, X, c, v, v_kind, y, y_user, y_kind, g->part);
}

void launch_pair(const dpcg_guess *g, int l, const double *coef, bool dot, hipStream_t s) {
    const int grid = (int)(g->ld / (kBlock * kGsRows));
    double *part = dot ? g->part : nullptr;
    hipLaunchKernelGGL((k_gs_pair<kGsRows>), dim3(grid), dim3(kBlock), 0, s, g->ld, l, g->X, g->W, coef, g->d, g->w, part);
}

void release_buffers(dpcg_guess *g) {
    dev_free(g->X);
    dev_free(g->W);
    dev_free(g->x0);
    dev_free(g->d);
    dev_free(g->w);
    dev_free(g->part);
    dev_free(g->coef);
}

void clear_state(dpcg_guess *g) {
    g->size = 0;
    g->c_valid = false;
    g->restarts = g->appended = g->skipped = g->dropped = g->reorthos = 0;
    if (g->h) g->epoch = g->h->values_epoch;
}

// The matrix has new values: W = A X~ again, then CholQR2 in the new A inner product (see the head of this file).
int reorthonormalise(dpcg_guess *g, hipStream_t s) {
    dpcg_system *h = g->h;
    int l = g->size;
    for (int j = 0; j < l; ++j) DPCG_TRY(dpcg_spmv(h, g->X + (int64_t)j * g->ld, g->W + (int64_t)j * g->ld, s));
    std::vector<double> G;
    const double tol2 = g->tol_dep * g->tol_dep;
    for (int round = 0; round < 2 && l > 0; ++round) {
        // column j of the Gram matrix: G[i][j] = <x~_i, W_j>, kept at G[j * l + i]
        for (int j = 0; j < l; ++j)
            gs_gram_column(g->ld, l, g->X, g->W + (int64_t)j * g->ld, g->part, g->coef + kCoefGram + j * l, s);
        DPCG_CHECK_LAUNCH();
        G.assign((size_t)l * l, 0.0);
        DPCG_HIP(hipMemcpyAsync(G.data(), g->coef + kCoefGram, (size_t)l * l * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        std::vector<double> &T = g->rinv_host;
        const int keep = gs_cholesky_rinv(G, l, tol2, T);
        g->dropped += l - keep;
        l = keep;
        if (l == 0) break;
        DPCG_HIP(hipMemcpyAsync(g->coef + kCoefRinv, T.data(), (size_t)l * l * sizeof(double), hipMemcpyHostToDevice, s));
        gs_rmul_pair(g->ld, l, g->X, g->W, g->coef + kCoefRinv, s);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipStreamSynchronize(s));      // (T is overwritten by the next round)
    }
    g->size = l;
    g->reorthos += 1;
    g->epoch = h->values_epoch;
    g->c_valid = false;
    return DPCG_OK;
}

int guess_state_error(const char *who) {
    set_error(std::string(who) + ": the system of this guess has been destroyed");
    return DPCG_ERR_STATE;
}

}  // namespace

// dpcg_destroy: the guesses of the handle lose their buffers and their system; the objects stay for dpcg_guess_destroy
void orphan_guesses(dpcg_system *h) {
    for (dpcg_guess *g : h->guesses) {
        release_buffers(g);
        g->h = nullptr;
        g->size = 0;
    }
    h->guesses.clear();
}

}  // namespace dpcg

// ---- the pieces of CholQR2 that dpcg_deflation.hip shares (dpcg_host.h) ----------------------------------------------------------
void gs_gram_column(int64_t ld, int l, const double *X, const double *v, double *part, double *out, hipStream_t s) {
    const int grid = (int)(ld / (kBlock * kGsRows));
    hipLaunchKernelGGL((k_gs_dots<kGsRows>), dim3(grid), dim3(kBlock), 0, s, ld, ld, l, X, v, (int)GS_PADDED, 0, part);
    if (l > 0) hipLaunchKernelGGL(k_gs_fin, dim3(l), dim3(kBlock), 0, s, part, ld / (64 * kGsRows), out);
}

int gs_cholesky_rinv(const std::vector<double> &G, int l, double tol2, std::vector<double> &T) {
    // G = R^T R from the upper triangle, row by row; sums over k ascending
    std::vector<double> R((size_t)l * l, 0.0);
    int keep = l;
    for (int j = 0; j < l; ++j) {
        const double gjj = G[(size_t)j * l + j];
        double p = gjj;
        for (int k = 0; k < j; ++k) p = p - R[(size_t)k * l + j] * R[(size_t)k * l + j];
        if (!std::isfinite(p) || !(p > tol2 * gjj)) {
            keep = j;
            break;
        }
        const double rjj = std::sqrt(p);
        R[(size_t)j * l + j] = rjj;
        for (int m = j + 1; m < l; ++m) {
            double t = G[(size_t)m * l + j];
            for (int k = 0; k < j; ++k) t = t - R[(size_t)k * l + j] * R[(size_t)k * l + m];
            R[(size_t)j * l + m] = t / rjj;
        }
    }
    // T = R^-1 of the leading keep x keep block, column by column (row-major, keep x keep)
    T.assign((size_t)keep * keep, 0.0);
    for (int j = 0; j < keep; ++j) {
        T[(size_t)j * keep + j] = 1.0 / R[(size_t)j * l + j];
        for (int i = j - 1; i >= 0; --i) {
            double t = 0.0;
            for (int k = i + 1; k <= j; ++k) t = t + R[(size_t)i * l + k] * T[(size_t)k * keep + j];
            T[(size_t)i * keep + j] = -t / R[(size_t)i * l + i];
        }
    }
    return keep;
}

void gs_rmul_pair(int64_t ld, int l, double *X, double *W, const double *rinv, hipStream_t s) {
    const dim3 grid((unsigned)(ld / (kBlock * 2)), 2);
    if (l <= 8) hipLaunchKernelGGL((k_gs_rmul<8>), grid, dim3(kBlock), 0, s, ld, l, X, W, rinv);
    else if (l <= 16) hipLaunchKernelGGL((k_gs_rmul<16>), grid, dim3(kBlock), 0, s, ld, l, X, W, rinv);
    else hipLaunchKernelGGL((k_gs_rmul<32>), grid, dim3(kBlock), 0, s, ld, l, X, W, rinv);
}

extern "C" int dpcg_guess_create(dpcg_handle_t h, int depth, double tol_dep, dpcg_guess_t *out) {
    if (!out) return invalid("dpcg_guess_create: out is NULL");
    *out = nullptr;
    if (!h) return invalid("dpcg_guess_create: NULL handle");
    if (depth < 1 || depth > kGsMaxDepth) return invalid("dpcg_guess_create: depth must lie in 1 .. 32");
    if (!(tol_dep > 0.0) || !std::isfinite(tol_dep)) return invalid("dpcg_guess_create: tol_dep must be positive and finite");
    const int64_t n = h->A.n;
    const int64_t ld = (n + kGsSpan - 1) / kGsSpan * kGsSpan;
    {
        // the basis, the three work vectors, the partials (one per 128 rows and column) and the scalars
        const double need = ((2.0 * depth + 3.0) * (double)ld + (depth + 1.0) * (double)(ld / (64 * kGsRows)) + kCoefCount) * sizeof(double);
        size_t free_b = 0, total_b = 0;
        DPCG_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > (double)free_b + (double)cached_memory_bytes()) {
            char buf[256];
            snprintf(buf, sizeof(buf), "dpcg_guess_create: the basis and its work vectors need %.2f GiB ((2 depth + 3) x n x 8 bytes, depth = %d, n = %lld), "
                     "%.2f GiB are free", need / 1073741824.0, depth, (long long)n, free_b / 1073741824.0);
            set_error(buf);
            return DPCG_ERR_NOMEM;
        }
    }
    SetupScope scope(nullptr);
    dpcg_guess *g = new dpcg_guess();
    g->h = h;
    g->depth = depth;
    g->tol_dep = tol_dep;
    g->n = n;
    g->ld = ld;
    g->nw = ld / (64 * kGsRows);
    std::fill(g->c_host, g->c_host + 32, 0.0);
    const int64_t basis = (int64_t)depth * ld;
    int st = DPCG_OK;
    if (((st = dev_alloc(&g->X, basis)) < 0 || (st = dev_alloc(&g->W, basis)) < 0) && st == DPCG_ERR_NOMEM)
        set_error("dpcg_guess_create: the basis (2 x depth x n doubles) does not fit in device memory");
    if (st >= 0) st = dev_alloc(&g->x0, ld);
    if (st >= 0) st = dev_alloc(&g->d, ld);
    if (st >= 0) st = dev_alloc(&g->w, ld);
    if (st >= 0) st = dev_alloc(&g->part, (int64_t)(depth + 1) * g->nw);
    if (st >= 0) st = dev_alloc(&g->coef, kCoefCount);
    const double one = 1.0;
    hipError_t e = hipSuccess;
    if (st >= 0) {
        // unwritten columns and the padding rows read as zero
        if (e == hipSuccess) e = hipMemsetAsync(g->X, 0, (size_t)basis * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemsetAsync(g->W, 0, (size_t)basis * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemsetAsync(g->x0, 0, (size_t)ld * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemsetAsync(g->d, 0, (size_t)ld * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemsetAsync(g->w, 0, (size_t)ld * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemsetAsync(g->coef, 0, (size_t)kCoefCount * sizeof(double), nullptr);
        if (e == hipSuccess) e = hipMemcpy(g->coef + kCoefOne, &one, sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) st = hip_fail(e, "dpcg_guess_create: clearing the basis", __FILE__, __LINE__);
    }
    if (st < 0) {
        release_buffers(g);
        delete g;
        return st;
    }
    g->epoch = h->values_epoch;
    h->guesses.push_back(g);
    *out = g;
    return DPCG_OK;
}

extern "C" int dpcg_guess_destroy(dpcg_guess_t g) {
    if (!g) return DPCG_OK;
    if (g->h) {
        SetupScope scope(nullptr, true);                  // (waits for the device: the basis may be in use on any stream)
        std::vector<dpcg_guess *> &v = g->h->guesses;
        v.erase(std::remove(v.begin(), v.end(), g), v.end());
        release_buffers(g);
    }
    delete g;
    return DPCG_OK;
}

extern "C" int dpcg_guess_reset(dpcg_guess_t g) {
    if (!g) return invalid("dpcg_guess_reset: NULL guess");
    if (!g->h) return guess_state_error("dpcg_guess_reset");
    clear_state(g);
    return DPCG_OK;
}

extern "C" int dpcg_guess_info(dpcg_guess_t g, int32_t out[8]) {
    if (!g || !out) return invalid("dpcg_guess_info: NULL argument");
    if (!g->h) return guess_state_error("dpcg_guess_info");
    out[0] = g->depth;
    out[1] = g->size;
    out[2] = g->restarts;
    out[3] = g->appended;
    out[4] = g->skipped;
    out[5] = g->dropped;
    out[6] = g->reorthos;
    out[7] = (int32_t)(g->epoch & 0x7fffffff);
    return DPCG_OK;
}

extern "C" int dpcg_guess_get_basis(dpcg_guess_t g, double *X_host, double *W_host) {
    if (!g) return invalid("dpcg_guess_get_basis: NULL guess");
    if (!g->h) return guess_state_error("dpcg_guess_get_basis");
    if (g->size == 0) return DPCG_OK;
    DPCG_HIP(device_wide_wait());                         // (no stream argument: whatever stream the last update ran on)
    const size_t width = (size_t)g->n * sizeof(double), pitch = (size_t)g->ld * sizeof(double);
    if (X_host) DPCG_HIP(hipMemcpy2D(X_host, width, g->X, pitch, width, (size_t)g->size, hipMemcpyDeviceToHost));
    if (W_host) DPCG_HIP(hipMemcpy2D(W_host, width, g->W, pitch, width, (size_t)g->size, hipMemcpyDeviceToHost));
    return DPCG_OK;
}

extern "C" int dpcg_guess_project(dpcg_guess_t g, const double *b, double *x0, dpcg_stream_t stream) {
    if (!g || !b || !x0) return invalid("dpcg_guess_project: NULL argument");
    if (!g->h) return guess_state_error("dpcg_guess_project");
    hipStream_t s = (hipStream_t)stream;
    if (g->epoch != g->h->values_epoch) DPCG_TRY(reorthonormalise(g, s));
    const int l = g->size;
    double ch[kGsMaxDepth + 1];
    launch_dots(g, l, g->X, b, user_kind(b), true, g->coef + kCoefG1, s);       // c[0 .. l), the probe of b behind it
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipMemcpyAsync(ch, g->coef + kCoefG1, (size_t)(l + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    bool finite = std::isfinite(ch[l]);
    for (int i = 0; i < l; ++i) finite = finite && std::isfinite(ch[i]);
    if (!finite) return invalid("dpcg_guess_project: b holds a non-finite value (or overflows against the basis)");
    launch_combine<0>(g, l, g->X, g->coef + kCoefG1, nullptr, GS_PADDED, g->x0, x0, s);
    DPCG_CHECK_LAUNCH();
    std::fill(g->c_host, g->c_host + kGsMaxDepth, 0.0);
    std::copy(ch, ch + l, g->c_host);
    g->c_valid = true;
    return DPCG_OK;
}

extern "C" int dpcg_guess_update(dpcg_guess_t g, const double *x, dpcg_stream_t stream) {
    if (!g || !x) return invalid("dpcg_guess_update: NULL argument");
    if (!g->h) return guess_state_error("dpcg_guess_update");
    hipStream_t s = (hipStream_t)stream;
    if (g->epoch != g->h->values_epoch) DPCG_TRY(reorthonormalise(g, s));
    const bool restart = g->size == g->depth;
    const int l = restart ? 0 : g->size;
    const bool use_x0 = !restart && g->c_valid;
    // d = x - x0 as "v - X c" with the one column x0 and c = 1 (bit for bit x - x0), and the probe of x
    launch_combine<1>(g, use_x0 ? 1 : 0, g->x0, g->coef + kCoefOne, x, user_kind(x), g->d, nullptr, s);
    hipLaunchKernelGGL(k_gs_fin, dim3(1), dim3(kBlock), 0, s, g->part, g->nw, g->coef + kCoefProbe);
    DPCG_CHECK_LAUNCH();
    DPCG_TRY(dpcg_spmv(g->h, g->d, g->w, s));
    if (l > 0) {
        launch_dots(g, l, g->X, g->w, GS_PADDED, false, g->coef + kCoefG1, s);
        launch_pair(g, l, g->coef + kCoefG1, false, s);
        launch_dots(g, l, g->X, g->w, GS_PADDED, false, g->coef + kCoefG2, s);
        launch_pair(g, l, g->coef + kCoefG2, true, s);
    } else {
        launch_pair(g, 0, g->coef + kCoefG1, true, s);
    }
    hipLaunchKernelGGL(k_gs_fin, dim3(1), dim3(kBlock), 0, s, g->part, g->nw, g->coef + kCoefS);
    DPCG_CHECK_LAUNCH();
    double ch[kCoefRead];
    DPCG_HIP(hipMemcpyAsync(ch, g->coef, sizeof(ch), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    if (!std::isfinite(ch[kCoefProbe])) return invalid("dpcg_guess_update: x holds a non-finite value");
    const double sdw = ch[kCoefS];
    double in_span = 0.0;                                  // |c + g|^2: the part of <x, A x> inside the span
    for (int i = 0; i < l; ++i) {
        const double e = ((use_x0 ? g->c_host[i] : 0.0) + ch[kCoefG1 + i]) + ch[kCoefG2 + i];
        in_span = in_span + e * e;
    }
    const double xax = in_span + sdw;
    if (!std::isfinite(sdw) || !(sdw > g->tol_dep * g->tol_dep * xax)) {
        g->skipped += 1;                                   // dependent: the basis (a full one too) stays as it is
        return DPCG_OK;
    }
    if (restart) {
        g->size = 0;
        g->restarts += 1;
        g->c_valid = false;
    } else {
        g->appended += 1;
    }
    const int grid = (int)(g->ld / (kBlock * kGsRows));
    double *xc = g->X + (int64_t)g->size * g->ld, *wc = g->W + (int64_t)g->size * g->ld;
    hipLaunchKernelGGL((k_gs_append<kGsRows>), dim3(grid), dim3(kBlock), 0, s, g->d, g->w, xc, wc, std::sqrt(sdw));
    DPCG_CHECK_LAUNCH();
    g->size += 1;
    return DPCG_OK;
}
