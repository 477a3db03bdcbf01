// Spectrum of the preconditioned operator M A by a Lanczos process on the device (dpcg_spectrum, include/dpcg.h): the extreme
// eigenvalues of M A, their error bounds and lambda_max / lambda_min -- the number test.py:111-113 reports as cond(M @ A), at
// sizes where M A cannot be formed densely.
//
// Algorithm.  M A is similar to the symmetric M^{1/2} A M^{1/2}; Lanczos runs in the M inner product, as the Lanczos process
// hidden inside PCG does.  Basis vectors r_j ("residual space") and z_j = M r_j, orthonormal as <r_i, z_j> = delta_ij.
//   start:  v_i = hash(seed, caller's row index of i) in [-1, 1) (splitmix64 of a counter, k_lz_start), generated in the
//           caller's numbering and gathered into the handle's; u = M v; r_0 = v / sqrt(<v, u>), z_0 = u / sqrt(<v, u>).
//   step j: w = A z_j;  alpha_j = <z_j, w>;  w -= alpha_j r_j + beta_j r_{j-1}  (beta_0 = 0);
//           full reorthogonalisation by classical Gram-Schmidt twice (CGS2): c = Z^T w, w -= R c, two passes;
//           u = M w;  beta_{j+1} = sqrt(<w, u>);  r_{j+1} = w / beta_{j+1}, z_{j+1} = u / beta_{j+1} (basis columns j + 1).
//   The eigenvalues theta of T_k = tridiag(beta, alpha, beta) are Ritz values of M A; a Ritz value's error bound is
//   beta_{k+1} |s_k|, s_k the last component of its eigenvector (dpcg_tridiag_ritz: implicit QL on the host).
//   Stop when both extreme bounds are <= rtol |theta|, when beta reaches 0 (invariant Krylov space: exact), after n steps
//   (the space is the whole space) or after max_steps.  <w, M w> < 0 (beyond rounding): M is not positive definite ->
//   DPCG_BREAKDOWN, no number.
//
// Layout.  R and Z are column-major with the column length padded to a multiple of 1024 rows (ld): every column starts
// 8 KiB-aligned, a lane owns 4 consecutive rows (two 16-byte loads per column; 1 row below 512 K rows, for parallelism), and the padding rows
// are zero (the basis is cleared at the start), so the vector kernels run over ld rows without bounds tests.  Column-major
// keeps the reorthogonalisation a pure stream of whole columns and lets SpMV / M read a basis column in place.
//
// Kernels of one step (after the SpMV, which sums the partials of alpha_j on the way, and before M):
//   k_lz_fin_alpha      alpha_j from the SpMV's partials (one workgroup, fixed order)
//   k_lz_update<0>      w -= alpha_j r_j + beta_j r_{j-1}, fused with the per-wave partials of c = Z^T w (columns 0..j)
//   k_lz_fin_cols       c[i] = sum of column i's partials, fixed order (one workgroup per column)
//   k_lz_update<1>      w -= R c, fused with the partials of the second pass's c = Z^T w
//   k_lz_fin_cols
//   k_lz_update<2>      w -= R c
//   (u = M w: apply_precond; <w, u>: launch_dot_partials)
//   k_lz_fin_beta       beta_{j+1}, the status word
//   k_lz_store          r_{j+1}, z_{j+1} into the basis
// No float atomics: every sum has one order, results are the same bits from run to run.  alpha, beta and the status stay in
// device memory; the host reads them every kCheckEvery steps.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"

namespace dpcg {
namespace {

constexpr int kLzRows = 4;                      // rows per lane of the store kernel, and of the update kernels at >= kLzWideRows rows
constexpr int kLzSpan = kBlock * kLzRows;       // rows per workgroup (1024): ld is a multiple of it
constexpr int64_t kLzWideRows = 1 << 19;        // smaller systems: one row per lane (4x the waves: a 22 K-row system fills 86 CUs, not 22)
constexpr int kCheckEvery = 16;                 // steps between host reads of alpha / beta

enum LzStatus { LZ_RUNNING = 0, LZ_INVARIANT = 1, LZ_NOT_SPD = 2, LZ_NONFINITE = 3 };
struct LzState {
    double norm0;   // sqrt(<v, M v>) of the start vector
    int status;     // LzStatus; once set every later kernel returns at once
    int stop;       // steps completed when the status was set
};

__device__ __forceinline__ double lz_hash(uint64_t seed, uint64_t i) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + (i + 1) * 0xBF58476D1CE4E5B9ull;   // splitmix64 finaliser of a counter
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// v[i] = hash(seed, caller's row of handle row i) for i < n, 0 in the padding
__global__ __launch_bounds__(kBlock) void k_lz_start(int64_t n, int64_t ld, uint64_t seed, const int32_t *__restrict__ perm,
                                                     double *__restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ld; i += stride)
        v[i] = i < n ? lz_hash(seed, (uint64_t)(perm ? perm[i] : i)) : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_lz_fin_alpha(const double *__restrict__ part, int n_part, double *__restrict__ alpha,
                                                         int j, const LzState *__restrict__ st) {
    __shared__ double sh[4];
    if (st->status) return;
    const double v = reduce_partials(part, n_part, sh);
    if (threadIdx.x == 0) alpha[j] = v;
}

// c[i] = sum over the nw partials of column i, in one fixed order (workgroup i)
__global__ __launch_bounds__(kBlock) void k_lz_fin_cols(const double *__restrict__ part, int64_t nw, double *__restrict__ c,
                                                        const LzState *__restrict__ st) {
    __shared__ double sh[4];
    if (st->status) return;
    const double *p = part + (int64_t)blockIdx.x * nw;
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < nw; k += kBlock) s += p[k];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) c[blockIdx.x] = s;
}

template <int ROWS>
__device__ __forceinline__ void lz_load(const double *p, double (&v)[ROWS]) {
    if constexpr (ROWS == 1) {
        v[0] = p[0];
    } else {
#pragma unroll
        for (int h = 0; h < ROWS / 2; ++h) {
            const double2 q = reinterpret_cast<const double2 *>(p)[h];
            v[2 * h] = q.x;
            v[2 * h + 1] = q.y;
        }
    }
}
template <int ROWS>
__device__ __forceinline__ void lz_store(double *p, const double (&v)[ROWS]) {
    if constexpr (ROWS == 1) {
        p[0] = v[0];
    } else {
#pragma unroll
        for (int h = 0; h < ROWS / 2; ++h) reinterpret_cast<double2 *>(p)[h] = make_double2(v[2 * h], v[2 * h + 1]);
    }
}

// MODE 0: w -= alpha_j r_j + beta_j r_{j-1}, then partials of Z^T w;  MODE 1: w -= R c, then partials;  MODE 2: w -= R c.
// Columns 0..j; a lane owns ROWS consecutive rows.  Grid: ld / (kBlock ROWS) workgroups, exact.  part[i * nw + wave] =
// <Z[:, i], w> over the wave's 64 ROWS rows (nw = ld / (64 ROWS)).
template <int MODE, int ROWS>
__global__ __launch_bounds__(kBlock) void k_lz_update(int64_t ld, int j, double *__restrict__ w, const double *__restrict__ R,
                                                      const double *__restrict__ Z, const double *__restrict__ c,
                                                      const double *__restrict__ alpha, const double *__restrict__ beta,
                                                      double *__restrict__ part, const LzState *__restrict__ st) {
    if (st->status) return;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t row = t * ROWS;
    double x[ROWS];
    lz_load<ROWS>(w + row, x);
    if (MODE == 0) {
        const double al = alpha[j];
        double r[ROWS];
        lz_load<ROWS>(R + (int64_t)j * ld + row, r);
#pragma unroll
        for (int k = 0; k < ROWS; ++k) x[k] = x[k] - al * r[k];
        if (j > 0) {
            const double be = beta[j];
            lz_load<ROWS>(R + (int64_t)(j - 1) * ld + row, r);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) x[k] = x[k] - be * r[k];
        }
    } else {
        double acc[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) acc[k] = 0.0;
#pragma unroll 8
        for (int i = 0; i <= j; ++i) {
            const double ci = c[i];
            double r[ROWS];
            lz_load<ROWS>(R + (int64_t)i * ld + row, r);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) acc[k] = acc[k] + ci * r[k];
        }
#pragma unroll
        for (int k = 0; k < ROWS; ++k) x[k] = x[k] - acc[k];
    }
    lz_store<ROWS>(w + row, x);
    if (MODE == 2) return;
    const int64_t nw = ld / (64 * ROWS);
    const int64_t wave = t >> 6;
    const bool writer = (threadIdx.x & 63) == 63;
    constexpr int U = ROWS == 1 ? 8 : 4;      // columns whose loads are in flight before their reductions
    int i = 0;
    for (; i + U <= j + 1; i += U) {
        double d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double z[ROWS];
            lz_load<ROWS>(Z + (int64_t)(i + u) * ld + row, z);
            d[u] = 0.0;
#pragma unroll
            for (int k = 0; k < ROWS; ++k) d[u] = d[u] + z[k] * x[k];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double s = wave_sum(d[u]);
            if (writer) part[(int64_t)(i + u) * nw + wave] = s;
        }
    }
    for (; i <= j; ++i) {
        double z[ROWS];
        lz_load<ROWS>(Z + (int64_t)i * ld + row, z);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) d = d + z[k] * x[k];
        const double s = wave_sum(d);
        if (writer) part[(int64_t)i * nw + wave] = s;
    }
}

// beta = sqrt(<w, M w>) into *slot.  first: the start vector (any value <= 0: M is not positive definite).  Otherwise a
// value <= 0 within rounding of the step's scale (alpha_j^2 + beta_j^2) means w vanished: the Krylov space is invariant.
__global__ __launch_bounds__(kBlock) void k_lz_fin_beta(const double *__restrict__ part, int n_part, double *__restrict__ slot,
                                                        const double *__restrict__ alpha, const double *__restrict__ beta, int j,
                                                        bool first, LzState *__restrict__ st) {
    __shared__ double sh[4];
    if (st->status) return;
    const double s = reduce_partials(part, n_part, sh);
    if (threadIdx.x != 0) return;
    const int steps = first ? 0 : j + 1;
    if (!isfinite(s)) {
        st->status = LZ_NONFINITE;
        st->stop = steps;
    } else if (s > 0.0) {
        *slot = sqrt(s);
    } else {
        const double scale = first ? 0.0 : alpha[j] * alpha[j] + beta[j] * beta[j];
        st->status = (!first && -s <= 1e-13 * scale) ? LZ_INVARIANT : LZ_NOT_SPD;
        st->stop = steps;
        if (st->status == LZ_INVARIANT) *slot = 0.0;
    }
}

// r_next = w / beta, z_next = u / beta over ld rows (the padding rows of w and u are zero)
__global__ __launch_bounds__(kBlock) void k_lz_store(const double *__restrict__ w, const double *__restrict__ u,
                                                     double *__restrict__ r_next, double *__restrict__ z_next,
                                                     const double *__restrict__ slot, const LzState *__restrict__ st) {
    if (st->status) return;
    const double be = *slot;
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kLzRows;
    const double2 *w2 = reinterpret_cast<const double2 *>(w + row);
    const double2 *u2 = reinterpret_cast<const double2 *>(u + row);
    double2 *r2 = reinterpret_cast<double2 *>(r_next + row);
    double2 *z2 = reinterpret_cast<double2 *>(z_next + row);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double2 a = w2[h], b = u2[h];
        r2[h] = make_double2(a.x / be, a.y / be);
        z2[h] = make_double2(b.x / be, b.y / be);
    }
}

// Ritz vectors y_i = Z s_i, i < nvec <= kLzVecMax: the tall-skinny product (n x m)(m x nvec) in one pass over the basis columns.  A lane
// owns 2 consecutive rows and keeps their kLzVecMax accumulators in registers; S (m x kLzVecMax, row-major, the unused columns zero) is
// staged through LDS kLzVecChunk rows at a time (every lane reads the same word: a broadcast); each sum runs over the basis columns in
// ascending order.  out: column-major n x nvec in the CALLER's numbering (perm: handle row -> caller row, or null).  Grid: ld / 512.
constexpr int kLzVecMax = 8, kLzVecChunk = 512;
__global__ __launch_bounds__(kBlock) void k_lz_ritz_vectors(int64_t ld, int64_t n, int m, const double *__restrict__ Z,
                                                            const double *__restrict__ S, int nvec, const int32_t *__restrict__ perm,
                                                            double *__restrict__ out) {
    __shared__ double sS[kLzVecChunk * kLzVecMax];
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
    double a0[kLzVecMax], a1[kLzVecMax];
#pragma unroll
    for (int j = 0; j < kLzVecMax; ++j) a0[j] = a1[j] = 0.0;
    for (int c0 = 0; c0 < m; c0 += kLzVecChunk) {
        const int cn = m - c0 < kLzVecChunk ? m - c0 : kLzVecChunk;
        __syncthreads();                                   // (the previous chunk may still be read)
        for (int t = threadIdx.x; t < cn * kLzVecMax; t += kBlock) sS[t] = S[(int64_t)c0 * kLzVecMax + t];
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < cn; ++c) {
            const double2 zv = *reinterpret_cast<const double2 *>(Z + (int64_t)(c0 + c) * ld + row);
#pragma unroll
            for (int j = 0; j < kLzVecMax; ++j) {
                const double sj = sS[c * kLzVecMax + j];
                a0[j] = a0[j] + zv.x * sj;
                a1[j] = a1[j] + zv.y * sj;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kLzVecMax; ++j) {
        if (j < nvec) {
            if (row < n) out[(int64_t)j * n + (perm ? perm[row] : row)] = a0[j];
            if (row + 1 < n) out[(int64_t)j * n + (perm ? perm[row + 1] : row + 1)] = a1[j];
        }
    }
}

struct LzBuffers {
    double *R = nullptr, *Z = nullptr, *w = nullptr, *u = nullptr, *part = nullptr, *part_s = nullptr, *part_d = nullptr;
    double *alpha = nullptr, *beta = nullptr, *c = nullptr, *S = nullptr;
    LzState *st = nullptr;
    ~LzBuffers() {
        dev_free(R);
        dev_free(Z);
        dev_free(w);
        dev_free(u);
        dev_free(part);
        dev_free(part_s);
        dev_free(part_d);
        dev_free(alpha);
        dev_free(beta);
        dev_free(c);
        dev_free(S);
        dev_free(st);
    }
};

}  // namespace
}  // namespace dpcg

// Eigenvalues of the symmetric tridiagonal T_k and the last row of its eigenvector matrix, by the implicit QL algorithm with
// Wilkinson shifts (Golub & Van Loan, Matrix Computations, section 8.3; the QL form deflates from the top).  Only the last row
// of the accumulated rotations is kept: O(k) work per sweep instead of O(k^2).  Ascending order.
extern "C" int dpcg_tridiag_ritz(int k, const double *alpha, const double *beta, double *theta, double *bottom) {
    if (k < 1 || !alpha || (k > 1 && !beta) || !theta || !bottom) return invalid("dpcg_tridiag_ritz: bad argument");
    std::vector<double> d(alpha, alpha + k), e(k, 0.0), z(k, 0.0);
    for (int i = 0; i + 1 < k; ++i) e[i] = beta[i];
    z[k - 1] = 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int l = 0; l < k; ++l) {
        for (int iter = 0;; ++iter) {
            int m = l;
            for (; m + 1 < k; ++m)                       // the first negligible off-diagonal at or below l splits the matrix
                if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
            if (m == l) break;
            if (iter == 60) return invalid("dpcg_tridiag_ritz: QL iteration did not converge");
            // shift: the eigenvalue of the leading 2 x 2 block closer to d[l]
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i = m - 1;
            bool underflow = false;
            for (; i >= l; --i) {                        // chase the bulge from the bottom of the block up to l
                const double f = s * e[i], b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) {                          // the rotation vanished: the block splits at i + 1
                    d[i + 1] -= p;
                    e[m] = 0.0;
                    underflow = true;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                const double zi1 = z[i + 1];             // the rotation on columns i, i + 1 of the eigenvector matrix, last row only
                z[i + 1] = s * z[i] + c * zi1;
                z[i] = c * z[i] - s * zi1;
            }
            if (underflow) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        }
    }
    std::vector<int> order(k);
    for (int i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
    for (int i = 0; i < k; ++i) {
        theta[i] = d[order[i]];
        bottom[i] = z[order[i]];
    }
    return DPCG_OK;
}

// The nvec lowest eigenpairs of the same tridiagonal as unit vectors: the QL iteration above with the rotations accumulated on the
// whole eigenvector matrix (O(k^2) per sweep; the eigenvalues take the same path and come out with the same bits).  S: column-major
// k x nvec, S[i * k + r] = component r of theta[i]'s eigenvector (sign arbitrary).
extern "C" int dpcg_tridiag_eigvecs(int k, const double *alpha, const double *beta, int nvec, double *theta, double *S) {
    if (k < 1 || !alpha || (k > 1 && !beta) || nvec < 1 || nvec > k || !theta || !S) return invalid("dpcg_tridiag_eigvecs: bad argument (1 <= nvec <= k)");
    std::vector<double> d(alpha, alpha + k), e(k, 0.0), V((size_t)k * k, 0.0);   // V[i * k + r]: component r of column i
    for (int i = 0; i + 1 < k; ++i) e[i] = beta[i];
    for (int i = 0; i < k; ++i) V[(size_t)i * k + i] = 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int l = 0; l < k; ++l) {
        for (int iter = 0;; ++iter) {
            int m = l;
            for (; m + 1 < k; ++m)
                if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
            if (m == l) break;
            if (iter == 60) return invalid("dpcg_tridiag_eigvecs: QL iteration did not converge");
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i = m - 1;
            bool underflow = false;
            for (; i >= l; --i) {
                const double f = s * e[i], b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) {
                    d[i + 1] -= p;
                    e[m] = 0.0;
                    underflow = true;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                double *vi = V.data() + (size_t)i * k, *vi1 = vi + k;       // the rotation on columns i, i + 1, every row
                for (int row = 0; row < k; ++row) {
                    const double t = vi1[row];
                    vi1[row] = s * vi[row] + c * t;
                    vi[row] = c * vi[row] - s * t;
                }
            }
            if (underflow) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0.0;
        }
    }
    std::vector<int> order(k);
    for (int i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
    for (int i = 0; i < nvec; ++i) {
        theta[i] = d[order[i]];
        std::copy(V.begin() + (size_t)order[i] * k, V.begin() + (size_t)(order[i] + 1) * k, S + (size_t)i * k);
    }
    return DPCG_OK;
}

// The Lanczos run behind dpcg_spectrum (nvec = 0: stops on the two extreme Ritz pairs) and dpcg_spectrum_vectors (nvec > 0: stops on
// the nvec lowest ones and leaves their Ritz vectors in W_dev before the basis is released).  `who` heads the error texts.
static int lanczos_run(dpcg_system *h, const char *who, int max_steps, double rtol, uint64_t seed, hipStream_t s, int nvec, int *steps,
                       double *theta_min, double *theta_max, double *err_min, double *err_max, double *alpha, double *beta,
                       double *theta_low, double *err_low, double *W_dev) {
    const std::string name(who);
    if (h->precond == DPCG_PRECOND_LU_MULTIPLY || h->precond == DPCG_PRECOND_LU_SOLVE) {
        // the process runs in the M inner product, which a non-symmetric M does not define: no step is taken
        if (steps) *steps = 0;
        set_error(name + ": M = L U is not symmetric");
        return DPCG_BREAKDOWN;
    }
    const int64_t n = h->A.n;
    const int m = (int)std::min<int64_t>(max_steps, n);  // the Krylov space has at most n dimensions
    const int64_t ld = (n + kLzSpan - 1) / kLzSpan * kLzSpan;
    const int rows = n >= kLzWideRows ? kLzRows : 1;        // rows per lane of the update kernels
    const int64_t nw = ld / (64 * rows);                   // partials per column: one per wave
    const int vgrid = (int)(ld / kLzSpan);
    const int ugrid = (int)(ld / (kBlock * rows));
    {
        const double need = 2.0 * (double)(m + 1) * (double)ld * sizeof(double);
        size_t free_b = 0, total_b = 0;
        DPCG_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > (double)free_b + (double)cached_memory_bytes()) {
            char buf[256];
            snprintf(buf, sizeof(buf), "%s: the Lanczos basis needs %.2f GiB (2 x (max_steps + 1) x n x 8 bytes, "
                     "max_steps = %d, n = %lld), %.2f GiB are free", who, need / 1073741824.0, m, (long long)n, free_b / 1073741824.0);
            set_error(buf);
            return DPCG_ERR_NOMEM;
        }
    }
    DPCG_TRY(ensure_work(h, 0, false, false));     // apply_precond's own scratch (t, q)
    SetupScope scope(s);
    LzBuffers B;
    const int64_t basis = (int64_t)(m + 1) * ld;
    {
        int st = DPCG_OK;
        if ((st = dev_alloc(&B.R, basis)) < 0 || (st = dev_alloc(&B.Z, basis)) < 0) {
            set_error(name + ": the Lanczos basis (2 x (max_steps + 1) x n doubles) does not fit in device memory");
            return st;
        }
    }
    DPCG_TRY(dev_alloc(&B.w, ld));
    DPCG_TRY(dev_alloc(&B.u, ld));
    DPCG_TRY(dev_alloc(&B.part, (int64_t)(m + 1) * nw));
    DPCG_TRY(dev_alloc(&B.part_s, kMaxSpmvGrid));
    DPCG_TRY(dev_alloc(&B.part_d, kMaxGrid));
    DPCG_TRY(dev_alloc(&B.alpha, m));
    DPCG_TRY(dev_alloc(&B.beta, m + 1));
    DPCG_TRY(dev_alloc(&B.c, m + 1));
    DPCG_TRY(dev_alloc(&B.st, 1));
    DPCG_HIP(hipMemsetAsync(B.R, 0, (size_t)basis * sizeof(double), s));   // unwritten columns and padding rows read as zero
    DPCG_HIP(hipMemsetAsync(B.Z, 0, (size_t)basis * sizeof(double), s));
    DPCG_HIP(hipMemsetAsync(B.w, 0, (size_t)ld * sizeof(double), s));
    DPCG_HIP(hipMemsetAsync(B.u, 0, (size_t)ld * sizeof(double), s));
    DPCG_HIP(hipMemsetAsync(B.alpha, 0, (size_t)m * sizeof(double), s));
    DPCG_HIP(hipMemsetAsync(B.beta, 0, (size_t)(m + 1) * sizeof(double), s));
    DPCG_HIP(hipMemsetAsync(B.st, 0, sizeof(LzState), s));
    const int dgrid = grid_for(n);

    // start vector: hashed in the caller's numbering, gathered into the handle's, normalised in the M inner product
    hipLaunchKernelGGL(k_lz_start, dim3(vgrid), dim3(kBlock), 0, s, n, ld, (unsigned long long)seed, h->perm, B.w);
    DPCG_TRY(apply_precond(h, B.w, B.u, s));
    launch_dot_partials(n, nullptr, B.w, B.u, B.part_d, dgrid, s);
    hipLaunchKernelGGL(k_lz_fin_beta, dim3(1), dim3(kBlock), 0, s, B.part_d, dgrid, &B.st->norm0, B.alpha, B.beta, 0, true, B.st);
    hipLaunchKernelGGL(k_lz_store, dim3(vgrid), dim3(kBlock), 0, s, B.w, B.u, B.R, B.Z, &B.st->norm0, B.st);
    DPCG_CHECK_LAUNCH();

    std::vector<double> ah(m), bh(m + 1), theta(m), bottom(m);
    LzState sh{};
    int k = 0;
    bool converged = false;
    double tmin = NAN, tmax = NAN, emin = NAN, emax = NAN;
    for (int j = 0; j < m; ++j) {
        const double *Zj = B.Z + (int64_t)j * ld;
        launch_spmv(h->A, h->planA, Zj, B.w, B.part_s, nullptr, s);                    // w = A z_j, partials of <z_j, w>
        hipLaunchKernelGGL(k_lz_fin_alpha, dim3(1), dim3(kBlock), 0, s, B.part_s, h->planA.grid, B.alpha, j, B.st);
        if (rows == 1) hipLaunchKernelGGL((k_lz_update<0, 1>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        else hipLaunchKernelGGL((k_lz_update<0, kLzRows>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        hipLaunchKernelGGL(k_lz_fin_cols, dim3(j + 1), dim3(kBlock), 0, s, B.part, nw, B.c, B.st);
        if (rows == 1) hipLaunchKernelGGL((k_lz_update<1, 1>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        else hipLaunchKernelGGL((k_lz_update<1, kLzRows>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        hipLaunchKernelGGL(k_lz_fin_cols, dim3(j + 1), dim3(kBlock), 0, s, B.part, nw, B.c, B.st);
        if (rows == 1) hipLaunchKernelGGL((k_lz_update<2, 1>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        else hipLaunchKernelGGL((k_lz_update<2, kLzRows>), dim3(ugrid), dim3(kBlock), 0, s, ld, j, B.w, B.R, B.Z, B.c, B.alpha, B.beta, B.part, B.st);
        DPCG_TRY(apply_precond(h, B.w, B.u, s));                                        // u = M w
        launch_dot_partials(n, nullptr, B.w, B.u, B.part_d, dgrid, s);
        hipLaunchKernelGGL(k_lz_fin_beta, dim3(1), dim3(kBlock), 0, s, B.part_d, dgrid, B.beta + j + 1, B.alpha, B.beta, j, false, B.st);
        hipLaunchKernelGGL(k_lz_store, dim3(vgrid), dim3(kBlock), 0, s, B.w, B.u, B.R + (int64_t)(j + 1) * ld, B.Z + (int64_t)(j + 1) * ld,
                           B.beta + j + 1, B.st);
        DPCG_CHECK_LAUNCH();
        const int done = j + 1;
        if (done % kCheckEvery != 0 && done != m) continue;
        DPCG_HIP(hipMemcpyAsync(&sh, B.st, sizeof(LzState), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipMemcpyAsync(ah.data(), B.alpha, (size_t)done * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipMemcpyAsync(bh.data(), B.beta, (size_t)(done + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        if (sh.status == LZ_NOT_SPD || sh.status == LZ_NONFINITE) {
            char buf[256];
            snprintf(buf, sizeof(buf), "%s: %s after %d steps: M is not symmetric positive definite, or A / M hold "
                     "non-finite values", who, sh.status == LZ_NOT_SPD ? "<w, M w> <= 0" : "a non-finite <w, M w>", sh.stop);
            set_error(buf);
            return DPCG_BREAKDOWN;
        }
        k = sh.status == LZ_INVARIANT ? sh.stop : done;
        if (k < 1) {
            set_error(name + ": the start vector lies in an invariant space of dimension 0");
            return DPCG_BREAKDOWN;
        }
        DPCG_TRY(dpcg_tridiag_ritz(k, ah.data(), bh.data() + 1, theta.data(), bottom.data()));
        const double bnext = bh[k];                      // beta_{k+1}
        tmin = theta[0];
        tmax = theta[k - 1];
        emin = bnext * std::fabs(bottom[0]);
        emax = bnext * std::fabs(bottom[k - 1]);
        bool small = emin <= rtol * std::fabs(tmin) && emax <= rtol * std::fabs(tmax);
        if (nvec > 0) {                                  // the nvec lowest pairs instead of the two extreme ones
            small = k >= nvec;
            for (int i = 0; small && i < nvec; ++i) small = bnext * std::fabs(bottom[i]) <= rtol * std::fabs(theta[i]);
        }
        converged = sh.status == LZ_INVARIANT || k == n || small;
        if (converged || sh.status) break;
    }
    if (steps) *steps = k;
    if (nvec > 0) {
        if (k < nvec) {
            char buf[200];
            snprintf(buf, sizeof(buf), "%s: the Krylov space of the start vector has %d dimensions, fewer than the %d vectors asked for", who, k, nvec);
            set_error(buf);
            return DPCG_ERR_INVALID;
        }
        std::vector<double> S((size_t)k * nvec), Sp((size_t)k * kLzVecMax, 0.0);
        DPCG_TRY(dpcg_tridiag_eigvecs(k, ah.data(), bh.data() + 1, nvec, theta_low, S.data()));
        for (int i = 0; i < nvec; ++i) {
            err_low[i] = bh[k] * std::fabs(S[(size_t)i * k + k - 1]);
            for (int r = 0; r < k; ++r) Sp[(size_t)r * kLzVecMax + i] = S[(size_t)i * k + r];
        }
        DPCG_TRY(dev_alloc(&B.S, (int64_t)k * kLzVecMax));
        DPCG_HIP(hipMemcpyAsync(B.S, Sp.data(), Sp.size() * sizeof(double), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_lz_ritz_vectors, dim3((unsigned)(ld / (kBlock * 2))), dim3(kBlock), 0, s, ld, n, k, B.Z, B.S, nvec, h->perm, W_dev);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipStreamSynchronize(s));               // (Sp and the basis go out of scope)
    }
    if (theta_min) *theta_min = tmin;
    if (theta_max) *theta_max = tmax;
    if (err_min) *err_min = emin;
    if (err_max) *err_max = emax;
    if (alpha) std::copy(ah.begin(), ah.begin() + k, alpha);
    if (beta) std::copy(bh.begin() + 1, bh.begin() + 1 + k, beta);
    return converged ? DPCG_OK : DPCG_MAX_ITER;
}

extern "C" int dpcg_spectrum(dpcg_handle_t h, int max_steps, double rtol, uint64_t seed, dpcg_stream_t stream, int *steps,
                             double *theta_min, double *theta_max, double *err_min, double *err_max, double *alpha,
                             double *beta) {
    if (!h || max_steps < 1 || !(rtol >= 0.0)) return invalid("dpcg_spectrum: bad argument (max_steps >= 1, rtol >= 0)");
    return lanczos_run(h, "dpcg_spectrum", max_steps, rtol, seed, (hipStream_t)stream, 0, steps, theta_min, theta_max, err_min, err_max, alpha,
                       beta, nullptr, nullptr, nullptr);
}

extern "C" int dpcg_spectrum_vectors(dpcg_handle_t h, int k, int max_steps, double rtol, uint64_t seed, dpcg_stream_t stream, int *steps,
                                     double *theta, double *err, double *W_dev) {
    if (!h || max_steps < 1 || !(rtol >= 0.0) || !theta || !err || !W_dev)
        return invalid("dpcg_spectrum_vectors: bad argument (max_steps >= 1, rtol >= 0, theta, err and W_dev not NULL)");
    if (k < 1 || k > kLzVecMax || k > h->A.n) return invalid("dpcg_spectrum_vectors: k must lie in 1 .. 8 and not exceed n");
    return lanczos_run(h, "dpcg_spectrum_vectors", max_steps, rtol, seed, (hipStream_t)stream, k, steps, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, theta, err, W_dev);
}
