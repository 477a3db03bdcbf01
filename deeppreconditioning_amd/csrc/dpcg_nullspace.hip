// Singular (symmetric positive SEMI-definite) systems: a null space attached to the handle and projected inside PCG
// (dpcg_set_nullspace / dpcg_get_nullspace, include/dpcg.h).  Not in the reference, whose systems are all definite.
// Compiled with -ffp-contract=off like dpcg_pcg.hip.
//
// Z is n x k with orthonormal columns (1 <= k <= 4), P = I - Z Z^T.  The solve (the contract is in include/dpcg.h):
//     b' = P b;  r = b' - A x0 (x0 given: r = P r once);  zt = M r;  s = Z^T zt;  t = Z^T r;  rho = <r,zt> - t^T s;  p = zt - Z s
//     update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  zt = M r (NOT projected in memory);
//              s = Z^T zt;  t = Z^T r;  rho' = <r,zt> - t^T s;  p = (zt - Z s) + (rho'/rho) p
//     end:     x = x - Z (Z^T x)
// Launches per update, M = I / Jacobi -- those of a definite solve in its three-kernel form:
//   K1   the handle's SpMV with its partials of <p,q> (launch_spmv with the iteration head: unchanged)
//   K2'  k_ns_update_r:   alpha;  r -= alpha q;  zt = dinv r on the fly;  per-workgroup partials of <r,r>, <r,zt>, Z^T zt, Z^T r
//   K3'  k_ns_update_xp:  the 2 + 2k sums re-reduced in one fixed order by every workgroup;  rho', beta;  workgroup 0 records the
//                         history and runs the test;  x += alpha p;  p = (zt - Z s) + beta p
// Any other M: K2' with <r,r> only, the handle's apply, k_ns_dots for the other 1 + 2k sums, K3'.
// CONST: Z = 1/sqrt(n), one column, never read -- K2' and K3' then move exactly the bytes of k_update_r / k_update_xp (40 per row
// each with Jacobi); a general Z adds 8k bytes per row to each pass.  All vectors are handle-owned: 16-byte accesses, the next pair
// requested before the current one is consumed.  No float atomics: wave tree, four wave sums in LDS, the partials in a fixed order.
// The control words (done, done_seen, k, the progress word) are the definite solve's (Scalars, record_and_test): the layout is
// untouched, the extra sums live in the null space's own partial buffer.
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_slots.h"

namespace dpcg {

constexpr int kNsMaxK = 4;
// partial slots, kMaxGrid doubles each: <r,r> (init: the first tested quantity), <r,zt>, Z^T zt (K of them), Z^T r (K), <b',b'>
constexpr int kNsSlotRR = 0, kNsSlotRZ = 1, kNsSlotS = 2;
constexpr int kNsSlots = 3 + 2 * kNsMaxK;

struct NullSpace {
    int k = 0;
    bool constant = false;          // Z = 1/sqrt(n): not stored
    double check_tol = 0.0;
    int64_t ld = 0;                 // column stride of Z: n rounded up to an even count (every column 16-byte aligned)
    double *Z = nullptr;            // device, k columns in the HANDLE's numbering (null when constant)
    std::vector<double> Z_host;     // the orthonormal basis, column-major n x k in the CALLER's numbering (empty when constant)
    double *bp = nullptr;           // b' = P b in the handle's numbering
    double *part = nullptr;         // kNsSlots x kMaxGrid
};

namespace {

// rows 2 i, 2 i + 1 of the K columns
template <int K, bool CONST>
__device__ __forceinline__ void z_load(const double *__restrict__ Z, int64_t ld, int64_t i, double2 (&zv)[K]) {
    if (CONST) return;
#pragma unroll
    for (int j = 0; j < K; ++j) zv[j] = reinterpret_cast<const double2 *>(Z + (int64_t)j * ld)[i];
}

// the sums re-reduced: Z^T zt and Z^T r scaled to the orthonormal Z (CONST: the plain sums times 1/sqrt(n)), and t^T s in column order
template <int K, bool CONST>
__device__ __forceinline__ double scale_and_dot(double (&s)[K], double (&t)[K], double zc) {
    double ts = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (CONST) {
            s[j] = zc * s[j];
            t[j] = zc * t[j];
        }
        ts += t[j] * s[j];
    }
    return ts;
}

// K2'.  PRE: 0 = M = I (zt = r), 1 = Jacobi (zt = dinv r, not stored: K3' forms the same product again), 2 = any other M (only
// r -= alpha q and <r,r>: the apply and k_ns_dots follow).
template <int K, bool CONST, int PRE>
__global__ __launch_bounds__(kBlock) void k_ns_update_r(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part_pq,
                                                        int n_part_pq, const double *__restrict__ q, double *__restrict__ r,
                                                        const double *__restrict__ dinv, const double *__restrict__ Z, int64_t ld,
                                                        double *__restrict__ part) {
    constexpr int N = PRE == 2 ? 1 : 2 + 2 * K;
    __shared__ double sh[4 * N > 8 ? 4 * N : 8];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ q2 = reinterpret_cast<const double2 *>(q);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ r2 = reinterpret_cast<double2 *>(r);
    double2 qa = make_double2(0, 0), ra = qa, da = qa, za[K];
#pragma unroll
    for (int j = 0; j < K; ++j) za[j] = qa;
    bool have = i < n2;
    if (have) {
        qa = q2[i];
        ra = r2[i];
        if (PRE == 1) da = d2[i];
        if (PRE != 2) z_load<K, CONST>(Z, ld, i, za);
    }
    // as k_update_r: the SpMV's partials, the `done` word and <r,z> travel with the first vector loads
    EarlyPartials<kSpmvPartSlots> ep;
    ep.request(part_pq, n_part_pq);
    const int done = sc->done;
    double rz_cur = sc->rz;
    pin_scalar(rz_cur);
    ep.land();
    if (done) return;
    const double pq = ep.reduce(n_part_pq, sh);
    const double alpha = rz_cur / pq;
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;         // read by K3' (a later kernel)
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    while (have) {
        const int64_t cur = i;
        const double2 qc = qa, rc = ra, dc = da;
        double2 zc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) zc[j] = za[j];
        i += stride;
        have = i < n2;
        if (have) {
            qa = q2[i];
            ra = r2[i];
            if (PRE == 1) da = d2[i];
            if (PRE != 2) z_load<K, CONST>(Z, ld, i, za);
        }
        double2 rn;
        rn.x = rc.x - alpha * qc.x;
        rn.y = rc.y - alpha * qc.y;
        r2[cur] = rn;
        acc[kNsSlotRR] += rn.x * rn.x;
        acc[kNsSlotRR] += rn.y * rn.y;
        if constexpr (PRE != 2) {
            double2 zn = rn;
            if (PRE == 1) {
                zn.x = dc.x * rn.x;
                zn.y = dc.y * rn.y;
            }
            acc[kNsSlotRZ] += rn.x * zn.x;
            acc[kNsSlotRZ] += rn.y * zn.y;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (CONST) {
                    acc[kNsSlotS + j] += zn.x;
                    acc[kNsSlotS + j] += zn.y;
                    acc[kNsSlotS + K + j] += rn.x;
                    acc[kNsSlotS + K + j] += rn.y;
                } else {
                    acc[kNsSlotS + j] += zc[j].x * zn.x;
                    acc[kNsSlotS + j] += zc[j].y * zn.y;
                    acc[kNsSlotS + K + j] += zc[j].x * rn.x;
                    acc[kNsSlotS + K + j] += zc[j].y * rn.y;
                }
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {               // odd tail element
        const int64_t e = n - 1;
        const double rn = r[e] - alpha * q[e];
        r[e] = rn;
        acc[kNsSlotRR] += rn * rn;
        if constexpr (PRE != 2) {
            const double zn = PRE == 1 ? dinv[e] * rn : rn;
            acc[kNsSlotRZ] += rn * zn;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double zj = CONST ? 1.0 : Z[(int64_t)j * ld + e];
                acc[kNsSlotS + j] += zj * zn;
                acc[kNsSlotS + K + j] += zj * rn;
            }
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) store_slots<N>(part, 0, acc);
}

// Partials of <r,zt>, Z^T zt, Z^T r for a zt that lies in memory (any M in the loop; the start of every solve).  init: also the
// first tested quantity -- <r,r> (init_check_r) or <zt,zt>, from which K_init takes s^T s -- and <b',b'>.  sc (loop only): skipped
// once the solve is done.
template <int K, bool CONST>
__global__ __launch_bounds__(kBlock) void k_ns_dots(int64_t n, const Scalars *__restrict__ sc, const double *__restrict__ r,
                                                    const double *__restrict__ zt, const double *__restrict__ bp,
                                                    const double *__restrict__ Z, int64_t ld, double *__restrict__ part, int init,
                                                    int init_check_r) {
    constexpr int N = 3 + 2 * K;                  // [0] first test, [1] <r,zt>, s, t, [2 + 2K] <b',b'>
    __shared__ double sh[4 * N];
    if (sc && sc->done) return;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ri = r[i], zi = zt[i];
        acc[kNsSlotRZ] += ri * zi;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double zj = CONST ? 1.0 : Z[(int64_t)j * ld + i];
            acc[kNsSlotS + j] += zj * zi;
            acc[kNsSlotS + K + j] += zj * ri;
        }
        if (init) {
            const double bi = bp[i];
            acc[kNsSlotRR] += init_check_r ? ri * ri : zi * zi;
            acc[2 + 2 * K] += bi * bi;
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < 2 + 2 * K; ++j) part[(int64_t)j * kMaxGrid + blockIdx.x] = acc[j];
        if (init) {
            part[(int64_t)kNsSlotRR * kMaxGrid + blockIdx.x] = acc[kNsSlotRR];
            part[(int64_t)(2 + 2 * K) * kMaxGrid + blockIdx.x] = acc[2 + 2 * K];
        }
    }
}

// Start of a solve: every workgroup re-reduces what k_ns_dots (init) left; p = zt - Z s; workgroup 0 sets up the control words and
// runs the first test -- on <p,p> = <zt,zt> - s^T s (the preconditioned residual the recurrence starts from), or on <r,r>.
template <int K, bool CONST>
__global__ __launch_bounds__(kBlock) void k_ns_init(int64_t n, Scalars *sc, const double *__restrict__ part, int G,
                                                    const double *__restrict__ zt, double *__restrict__ p,
                                                    const double *__restrict__ Z, int64_t ld, double zc, double rtol_sq,
                                                    double atol_sq, double *hist, int hist_cap, unsigned long long *progress,
                                                    int init_check_r) {
    constexpr int N = 3 + 2 * K;
    __shared__ double sh[4 * N];
    double v[N], s[K], t[K];
    reduce_slots<N>(part, 0, G, v, sh);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        s[j] = v[kNsSlotS + j];
        t[j] = v[kNsSlotS + K + j];
    }
    const double ts = scale_and_dot<K, CONST>(s, t, zc);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double pi = zt[i];
#pragma unroll
        for (int j = 0; j < K; ++j) pi = pi - (CONST ? zc : Z[(int64_t)j * ld + i]) * s[j];
        p[i] = pi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double rho = v[kNsSlotRZ] - ts;
        double tt = v[kNsSlotRR];
        if (!init_check_r) {
#pragma unroll
            for (int j = 0; j < K; ++j) tt = tt - s[j] * s[j];
        }
        sc->bb = v[2 + 2 * K];
        sc->rz = rho;
        sc->alpha = 0.0;
        sc->rtol_sq = rtol_sq;
        sc->atol_sq = atol_sq;
        sc->done = 0;
        sc->status = DPCG_MAX_ITER;
        sc->done_seen = 0;
        sc->progress = progress;
        record_and_test(sc, tt, rho, hist, hist_cap, 0);
    }
}

// K3'.  zsrc: r for PRE 0 and 1 (Jacobi: times dinv, the product K2' summed), the stored zt for PRE 2.
template <int K, bool CONST, int PRE>
__global__ __launch_bounds__(kBlock) void k_ns_update_xp(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part, int G,
                                                         const double *__restrict__ zsrc, const double *__restrict__ dinv,
                                                         double *__restrict__ p, double *__restrict__ x,
                                                         const double *__restrict__ Z, int64_t ld, double zc, double *__restrict__ hist,
                                                         int hist_cap) {
    constexpr int N = 2 + 2 * K;
    __shared__ double sh[4 * N];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ z2 = reinterpret_cast<const double2 *>(zsrc);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ p2 = reinterpret_cast<double2 *>(p);
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    double2 ta = make_double2(0, 0), pa = ta, xa = ta, da = ta, za[K];
#pragma unroll
    for (int j = 0; j < K; ++j) za[j] = ta;
    bool have = i < n2;
    if (have) {
        ta = z2[i];
        pa = p2[i];
        xa = x2[i];
        if (PRE == 1) da = d2[i];
        z_load<K, CONST>(Z, ld, i, za);
    }
    // `done_seen`, not `done` (see k_update_xp): workgroup 0 of THIS launch sets `done`
    const int done_seen = sc->done_seen;
    double rz_old = sc->rz, alpha = sc->alpha;
    pin_scalar(rz_old);
    pin_scalar(alpha);
    if (done_seen) return;
    double v[N], s[K], t[K];
    reduce_slots<N>(part, 0, G, v, sh);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        s[j] = v[kNsSlotS + j];
        t[j] = v[kNsSlotS + K + j];
    }
    const double rz_new = v[kNsSlotRZ] - scale_and_dot<K, CONST>(s, t, zc);      // <r, P zt>
    const double beta = rz_new / rz_old;
    if (blockIdx.x == 0 && threadIdx.x == 0) record_and_test(sc, v[kNsSlotRR], rz_new, hist, hist_cap, sc->k + 1);
    while (have) {
        const int64_t cur = i;
        double2 tc = ta;
        const double2 pc = pa, xc = xa, dc = da;
        double2 zv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) zv[j] = za[j];
        i += stride;
        have = i < n2;
        if (have) {
            ta = z2[i];
            pa = p2[i];
            xa = x2[i];
            if (PRE == 1) da = d2[i];
            z_load<K, CONST>(Z, ld, i, za);
        }
        if (PRE == 1) {                                                 // zt = dinv r, recomputed
            tc.x = dc.x * tc.x;
            tc.y = dc.y * tc.y;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {                                   // zt - Z s, columns ascending
            tc.x = tc.x - (CONST ? zc : zv[j].x) * s[j];
            tc.y = tc.y - (CONST ? zc : zv[j].y) * s[j];
        }
        double2 xn, pn;
        xn.x = xc.x + alpha * pc.x;
        xn.y = xc.y + alpha * pc.y;
        pn.x = tc.x + beta * pc.x;
        pn.y = tc.y + beta * pc.y;
        x2[cur] = xn;
        p2[cur] = pn;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t e = n - 1;
        const double pe = p[e];
        x[e] = x[e] + alpha * pe;
        double te = PRE == 1 ? dinv[e] * zsrc[e] : zsrc[e];
#pragma unroll
        for (int j = 0; j < K; ++j) te = te - (CONST ? zc : Z[(int64_t)j * ld + e]) * s[j];
        p[e] = te + beta * pe;
    }
}

// partials of Z^T v into slots kNsSlotS .. + K
template <int K, bool CONST>
__global__ __launch_bounds__(kBlock) void k_ns_zt_dots(int64_t n, const double *__restrict__ v, const double *__restrict__ Z, int64_t ld,
                                                       double *__restrict__ part) {
    __shared__ double sh[4 * K];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double vi = v[i];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += (CONST ? 1.0 : Z[(int64_t)j * ld + i]) * vi;
    }
    block_sum_n<K>(acc, sh);
    if (threadIdx.x == 0) store_slots<K>(part, kNsSlotS, acc);
}

// out = in - Z (Z^T in) from those partials (out may be in)
template <int K, bool CONST>
__global__ __launch_bounds__(kBlock) void k_ns_project(int64_t n, const double *in, double *out, const double *__restrict__ Z, int64_t ld,
                                                       double zc, const double *__restrict__ part, int G) {
    __shared__ double sh[4 * K];
    double c[K];
    reduce_slots<K>(part, kNsSlotS, G, c, sh);
    if (CONST) c[0] = zc * c[0];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double vi = in[i];
#pragma unroll
        for (int j = 0; j < K; ++j) vi = vi - (CONST ? zc : Z[(int64_t)j * ld + i]) * c[j];
        out[i] = vi;
    }
}

// ---- the check of A Z = 0 (setup): workgroup maxima, the host takes the maximum of those -------------------------------------
__device__ __forceinline__ double block_max(double v, double *sh) {      // sh: kBlock doubles; valid in thread 0
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    return sh[0];
}
// out[b] = max over the workgroup's rows of sum_k |a_ik|  (||A||_inf = the maximum over b)
__global__ __launch_bounds__(kBlock) void k_ns_row_abs_max(int64_t n, const int32_t *__restrict__ rp, const double *__restrict__ val,
                                                           double *__restrict__ out) {
    __shared__ double sh[kBlock];
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double s = 0.0;
        for (int k = rp[i]; k < rp[i + 1]; ++k) s += fabs(val[k]);
        m = fmax(m, s);
    }
    m = block_max(m, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}
// out[b] = max |v_i| over the workgroup's rows; a NaN in v comes out as +inf (fmax would drop it)
__global__ __launch_bounds__(kBlock) void k_ns_abs_max(int64_t n, const double *__restrict__ v, double *__restrict__ out) {
    __shared__ double sh[kBlock];
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double a = fabs(v[i]);
        m = (a == a) ? fmax(m, a) : __builtin_huge_val();
    }
    m = block_max(m, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}
__global__ __launch_bounds__(kBlock) void k_ns_fill(int64_t n, double value, double *__restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) v[i] = value;
}

// one kernel variant per shape of Z: the constant column, or 1 .. 4 stored ones
#define DPCG_NS_SHAPES(ns, LAUNCH)                   \
    do {                                             \
        if ((ns)->constant) { LAUNCH(1, true); }     \
        else if ((ns)->k == 1) { LAUNCH(1, false); } \
        else if ((ns)->k == 2) { LAUNCH(2, false); } \
        else if ((ns)->k == 3) { LAUNCH(3, false); } \
        else { LAUNCH(4, false); }                   \
    } while (0)

inline double z_const(const dpcg_system *h) { return 1.0 / std::sqrt((double)h->A.n); }

// v <- v - Z (Z^T v), or out = in - Z (Z^T in)
void launch_project(const dpcg_system *h, const double *in, double *out, hipStream_t s) {
    const NullSpace *ns = h->ns;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
#define DPCG_NS_L(KV, CV)                                                                                                    \
    hipLaunchKernelGGL((k_ns_zt_dots<KV, CV>), dim3(G), dim3(kBlock), 0, s, n, in, ns->Z, ns->ld, ns->part);                   \
    hipLaunchKernelGGL((k_ns_project<KV, CV>), dim3(G), dim3(kBlock), 0, s, n, in, out, ns->Z, ns->ld, z_const(h), ns->part, G)
    DPCG_NS_SHAPES(ns, DPCG_NS_L);
#undef DPCG_NS_L
}

void launch_ns_dots(const dpcg_system *h, const Scalars *sc, const double *r, const double *zt, bool init, int init_check_r, hipStream_t s) {
    const NullSpace *ns = h->ns;
#define DPCG_NS_L(KV, CV)                                                                                                        \
    hipLaunchKernelGGL((k_ns_dots<KV, CV>), dim3(h->vec_grid), dim3(kBlock), 0, s, h->A.n, sc, r, zt, ns->bp, ns->Z, ns->ld, ns->part, \
                       init ? 1 : 0, init_check_r)
    DPCG_NS_SHAPES(ns, DPCG_NS_L);
#undef DPCG_NS_L
}

inline int ns_pre(const dpcg_system *h) { return h->precond == DPCG_PRECOND_NONE ? 0 : (h->precond == DPCG_PRECOND_JACOBI ? 1 : 2); }

// one update as launches on s
int enqueue_ns_update(dpcg_system *h, hipStream_t s) {
    const NullSpace *ns = h->ns;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    const int pre = ns_pre(h);
    const double zc = z_const(h);
    IterCtl ctl{h->scal};
    launch_spmv(h->A, h->planA, h->p, h->q, h->part_pq, &ctl, s);                                // K1
#define DPCG_NS_K2(KV, CV)                                                                                                        \
    do {                                                                                                                          \
        if (pre == 0)                                                                                                             \
            hipLaunchKernelGGL((k_ns_update_r<KV, CV, 0>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, ns->Z, ns->ld, ns->part);                                                           \
        else if (pre == 1)                                                                                                        \
            hipLaunchKernelGGL((k_ns_update_r<KV, CV, 1>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, ns->Z, ns->ld, ns->part);                                                           \
        else                                                                                                                      \
            hipLaunchKernelGGL((k_ns_update_r<KV, CV, 2>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, ns->Z, ns->ld, ns->part);                                                           \
    } while (0)
    DPCG_NS_SHAPES(ns, DPCG_NS_K2);                                                               // K2'
#undef DPCG_NS_K2
    if (pre == 2) {
        DPCG_TRY(apply_precond(h, h->r, h->z, s, true));
        launch_ns_dots(h, h->scal, h->r, h->z, false, 0, s);
    }
#define DPCG_NS_K3(KV, CV)                                                                                                          \
    do {                                                                                                                            \
        if (pre == 0)                                                                                                               \
            hipLaunchKernelGGL((k_ns_update_xp<KV, CV, 0>), dim3(G), dim3(kBlock), 0, s, n, h->scal, ns->part, G, h->r, h->dinv, h->p, \
                               h->x, ns->Z, ns->ld, zc, h->hist, h->hist_cap);                                                      \
        else if (pre == 1)                                                                                                          \
            hipLaunchKernelGGL((k_ns_update_xp<KV, CV, 1>), dim3(G), dim3(kBlock), 0, s, n, h->scal, ns->part, G, h->r, h->dinv, h->p, \
                               h->x, ns->Z, ns->ld, zc, h->hist, h->hist_cap);                                                      \
        else                                                                                                                        \
            hipLaunchKernelGGL((k_ns_update_xp<KV, CV, 2>), dim3(G), dim3(kBlock), 0, s, n, h->scal, ns->part, G, h->z, h->dinv, h->p, \
                               h->x, ns->Z, ns->ld, zc, h->hist, h->hist_cap);                                                      \
    } while (0)
    DPCG_NS_SHAPES(ns, DPCG_NS_K3);                                                               // K3'
#undef DPCG_NS_K3
    return DPCG_OK;
}

void release(NullSpace *ns) {
    if (!ns) return;
    dev_free(ns->Z);
    dev_free(ns->bp);
    dev_free(ns->part);
    delete ns;
}

// max_i |(A z_j)_i| <= tol ||A||_inf ||z_j||_inf for every column (p, q of the handle are the scratch)
int check_columns(dpcg_system *h, const NullSpace *ns, const std::vector<double> &col_inf, hipStream_t s) {
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    DPCG_TRY(ensure_work(h, 0, false, false));
    std::vector<double> host((size_t)2 * kMaxGrid, 0.0);
    hipLaunchKernelGGL(k_ns_row_abs_max, dim3(G), dim3(kBlock), 0, s, n, h->A.rowptr, h->A.val, ns->part);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipMemcpyAsync(host.data(), ns->part, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    double norm_a = 0.0;
    for (int i = 0; i < G; ++i) norm_a = std::max(norm_a, host[(size_t)i]);
    for (int j = 0; j < ns->k; ++j) {
        const double *zj = ns->constant ? h->p : ns->Z + (int64_t)j * ns->ld;
        if (ns->constant) hipLaunchKernelGGL(k_ns_fill, dim3(G), dim3(kBlock), 0, s, n, z_const(h), h->p);
        launch_spmv(h->A, h->planA, zj, h->q, nullptr, nullptr, s);
        hipLaunchKernelGGL(k_ns_abs_max, dim3(G), dim3(kBlock), 0, s, n, h->q, ns->part);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipMemcpyAsync(host.data(), ns->part, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        double az = 0.0;
        for (int i = 0; i < G; ++i) az = std::max(az, host[(size_t)i]);
        const double bound = ns->check_tol * norm_a * col_inf[(size_t)j];
        if (!(az <= bound)) {
            char buf[320];
            snprintf(buf, sizeof(buf), "dpcg_set_nullspace: column %d is not in the null space of A: max |A z| = %.3e exceeds check_tol * ||A||_inf * "
                     "||z||_inf = %.3e (check_tol = %.1e)", j, az, bound, ns->check_tol);
            set_error(buf);
            return DPCG_ERR_INVALID;
        }
    }
    return DPCG_OK;
}

std::vector<double> column_inf_norms(const dpcg_system *h, const NullSpace *ns) {
    std::vector<double> out((size_t)ns->k, 0.0);
    const int64_t n = h->A.n;
    if (ns->constant) {
        out[0] = z_const(h);
        return out;
    }
    for (int j = 0; j < ns->k; ++j)
        for (int64_t i = 0; i < n; ++i) out[(size_t)j] = std::max(out[(size_t)j], std::fabs(ns->Z_host[(size_t)j * n + i]));
    return out;
}

}  // namespace
}  // namespace dpcg

void free_nullspace(dpcg_system *h) {
    release(h->ns);
    h->ns = nullptr;
}

const char *nullspace_refusal(const dpcg_system *h, int flags, const double *x_true) {
    if (!h->ns) return nullptr;
    if (flags & DPCG_SINGLE_REDUCTION) return "dpcg_solve: DPCG_SINGLE_REDUCTION is not available on a handle with a null space (the projected recurrence is the standard one)";
    if (flags & DPCG_SPMV_F32) return "dpcg_solve: DPCG_SPMV_F32 is not available on a handle with a null space";
    if (flags & DPCG_TEAM) return "dpcg_solve: DPCG_TEAM is not available on a handle with a null space (no one-launch form projects)";
    if (x_true) return "dpcg_solve: x_true tracking is not available on a handle with a null space (the solution is determined up to the null space)";
    if (h->precond == DPCG_PRECOND_AMG)
        return "dpcg_solve: the AMG preconditioner cannot serve a handle with a null space: its exact coarse solve inverts a singular matrix";
    if (h->precond == DPCG_PRECOND_CALLBACK)
        return "dpcg_solve: the callback preconditioner is not available on a handle with a null space";
    return nullptr;
}

// dpcg_update_values: the null space stays; a check that was asked for is repeated on the new values
int nullspace_values_changed(dpcg_system *h, hipStream_t s) {
    NullSpace *ns = h->ns;
    if (!ns || !(ns->check_tol > 0.0)) return DPCG_OK;
    const int st = check_columns(h, ns, column_inf_norms(h, ns), s);
    if (st == DPCG_ERR_INVALID) {
        std::string msg = dpcg_last_error();
        const std::string from = "dpcg_set_nullspace";
        if (msg.compare(0, from.size(), from) == 0) msg.replace(0, from.size(), "dpcg_update_values (the null space has been dropped)");
        free_nullspace(h);
        set_error(msg);
    }
    return st;
}

extern "C" int dpcg_set_nullspace(dpcg_handle_t h, int k, const double *Z, int memspace, double check_tol, dpcg_stream_t stream) {
    if (!h) return invalid("dpcg_set_nullspace: NULL handle");
    if (k < 0 || k > kNsMaxK) return invalid("dpcg_set_nullspace: k must lie in 0 .. 4 (0 clears)");
    if (k > 0 && h->df) return invalid("dpcg_set_nullspace: the handle has a deflation attached (dpcg_set_deflation): one or the other");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);            // (the old basis may be in use on another stream)
    if (k == 0) {
        free_nullspace(h);
        return DPCG_OK;
    }
    if (!Z && k != 1) return invalid("dpcg_set_nullspace: Z == NULL means the constant vector and needs k == 1");
    if (memspace != DPCG_HOST && memspace != DPCG_DEVICE) return invalid("dpcg_set_nullspace: bad memspace");
    if (!(check_tol == check_tol)) return invalid("dpcg_set_nullspace: check_tol is NaN");
    const int64_t n = h->A.n;
    NullSpace *ns = new NullSpace();
    ns->k = k;
    ns->constant = Z == nullptr;
    ns->check_tol = check_tol;
    ns->ld = (n + 1) & ~(int64_t)1;
    auto fail = [&](int st) {
        release(ns);
        return st;
    };
    int st = DPCG_OK;
    if (!ns->constant) {
        std::vector<double> &Q = ns->Z_host;
        Q.resize((size_t)n * k);
        if (memspace == DPCG_HOST) {
            memcpy(Q.data(), Z, Q.size() * sizeof(double));
        } else {
            hipError_t e = hipMemcpyAsync(Q.data(), Z, Q.size() * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_nullspace: reading Z", __FILE__, __LINE__));
        }
        for (size_t i = 0; i < Q.size(); ++i)
            if (!std::isfinite(Q[i])) return fail(invalid("dpcg_set_nullspace: Z holds a non-finite entry"));
        // modified Gram-Schmidt in fp64, every column orthogonalised twice against the ones before it
        auto dot = [&](const double *a, const double *b) {
            double acc = 0.0;
            for (int64_t i = 0; i < n; ++i) acc += a[i] * b[i];
            return acc;
        };
        for (int j = 0; j < k; ++j) {
            double *cj = Q.data() + (size_t)j * n;
            const double before = std::sqrt(dot(cj, cj));
            for (int pass = 0; pass < 2; ++pass)
                for (int i = 0; i < j; ++i) {
                    const double *ci = Q.data() + (size_t)i * n;
                    const double c = dot(ci, cj);
                    for (int64_t r = 0; r < n; ++r) cj[r] -= c * ci[r];
                }
            const double after = std::sqrt(dot(cj, cj));
            if (!std::isfinite(after) || !(after > 1e-12 * before)) {
                char buf[200];
                snprintf(buf, sizeof(buf), "dpcg_set_nullspace: Z is rank deficient: column %d has norm %.3e after orthogonalisation, %.3e before", j,
                         after, before);
                set_error(buf);
                return fail(DPCG_ERR_INVALID);
            }
            for (int64_t r = 0; r < n; ++r) cj[r] /= after;
        }
        // to the handle's numbering (row i of the handle = row perm[i] of the caller), columns ld apart, the padding row zero
        std::vector<double> Zp((size_t)ns->ld * k, 0.0);
        if (h->perm) {
            std::vector<int32_t> perm((size_t)n);
            hipError_t e = hipMemcpyAsync(perm.data(), h->perm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_nullspace: reading the permutation", __FILE__, __LINE__));
            for (int j = 0; j < k; ++j)
                for (int64_t i = 0; i < n; ++i) Zp[(size_t)j * ns->ld + i] = Q[(size_t)j * n + perm[(size_t)i]];
        } else {
            for (int j = 0; j < k; ++j) memcpy(Zp.data() + (size_t)j * ns->ld, Q.data() + (size_t)j * n, (size_t)n * sizeof(double));
        }
        if ((st = dev_alloc(&ns->Z, ns->ld * k)) < 0) return fail(st);
        hipError_t e = hipMemcpyAsync(ns->Z, Zp.data(), Zp.size() * sizeof(double), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);       // (Zp goes out of scope)
        if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_nullspace: uploading Z", __FILE__, __LINE__));
    }
    if ((st = dev_alloc(&ns->bp, n)) < 0) return fail(st);
    if ((st = dev_alloc(&ns->part, (int64_t)kNsSlots * kMaxGrid)) < 0) return fail(st);
    if (check_tol > 0.0 && (st = check_columns(h, ns, column_inf_norms(h, ns), s)) < 0) return fail(st);
    free_nullspace(h);
    h->ns = ns;
    return DPCG_OK;
}

extern "C" int dpcg_get_nullspace(dpcg_handle_t h, int *k, double *Z_host) {
    if (!h || !k) return invalid("dpcg_get_nullspace: NULL argument");
    const NullSpace *ns = h->ns;
    *k = ns ? ns->k : 0;
    if (!ns || !Z_host) return DPCG_OK;
    const int64_t n = h->A.n;
    if (ns->constant) {
        const double zc = z_const(h);
        for (int64_t i = 0; i < n; ++i) Z_host[i] = zc;
    } else {
        memcpy(Z_host, ns->Z_host.data(), ns->Z_host.size() * sizeof(double));
    }
    return DPCG_OK;
}

// The solve of a handle with a null space, whatever its size: plain launches enqueued ahead of the progress word that K3' posts
// (the kernels of an update enqueued beyond the stop return at once, as in the definite driver).
int solve_nullspace_one(dpcg_system *h, SolveCall c) {
    NullSpace *ns = h->ns;
    const int64_t n = h->A.n;
    hipStream_t s = c.s;
    const int G = h->vec_grid;
    const double zc = z_const(h);
    HandleExtras &ex = extras()[h];
    DPCG_TRY(ensure_work(h, c.max_iter, false, false));
    *ex.prog_host = 0;
    const double *b = c.b;
    if (h->perm) {                         // b and x0 arrive in the caller's numbering
        if (!h->pb) DPCG_TRY(dev_alloc(&h->pb, n));
        launch_gather_f64(n, h->perm, b, h->pb, s);
        b = h->pb;
    }
    launch_project(h, b, ns->bp, s);                                                   // b' = P b
    if (c.x0) {
        if (h->perm) launch_gather_f64(n, h->perm, c.x0, h->x, s);
        else DPCG_HIP(hipMemcpyAsync(h->x, c.x0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        launch_spmv(h->A, h->planA, h->x, h->q, nullptr, nullptr, s);
        launch_residual(n, ns->bp, h->q, h->r, G, s);                                  // r = b' - A x0
        launch_project(h, h->r, h->r, s);                                              // r = P r, once
    } else {
        DPCG_HIP(hipMemsetAsync(h->x, 0, (size_t)n * sizeof(double), s));
        DPCG_HIP(hipMemcpyAsync(h->r, ns->bp, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    const double *zt = h->precond == DPCG_PRECOND_NONE ? h->r : h->z;
    if (h->precond != DPCG_PRECOND_NONE) DPCG_TRY(apply_precond(h, h->r, h->z, s));
    const int init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    launch_ns_dots(h, nullptr, h->r, zt, true, init_check_r, s);
#define DPCG_NS_L(KV, CV)                                                                                                      \
    hipLaunchKernelGGL((k_ns_init<KV, CV>), dim3(G), dim3(kBlock), 0, s, n, h->scal, ns->part, G, zt, h->p, ns->Z, ns->ld, zc,    \
                       c.rtol_sq, c.atol_sq, h->hist, h->hist_cap, ex.prog_dev, init_check_r)
    DPCG_NS_SHAPES(ns, DPCG_NS_L);
#undef DPCG_NS_L
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();
    volatile unsigned long long *prog = ex.prog_host;
    int enq = 0;
    double t_iter = 0.0;
    for (;;) {
        const unsigned long long v = *prog;
        const int k = (int)(v >> 1);
        if ((v & 1ull) || k >= c.max_iter) break;
        if (k >= 4) t_iter = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / k;
        // updates kept enqueued beyond the last one reported: enough to cover ~150 us of host latency
        int ahead = 16;
        if (t_iter > 0.0) ahead = std::min(32, std::max(3, (int)(150e-6 / t_iter) + 2));
        while (enq < c.max_iter && enq - k < ahead) {
            DPCG_TRY(enqueue_ns_update(h, s));
            enq += 1;
        }
        DPCG_CHECK_LAUNCH();
        // wait for the progress word to move; watch the stream so that a fault cannot hang the host
        bool moved = false;
        for (int spin = 0; spin < 4000 && !moved; ++spin) {
            moved = *prog != v;
            if (!moved) __builtin_ia32_pause();
        }
        if (moved) continue;
        const hipError_t q = hipStreamQuery(s);
        if (q == hipErrorNotReady) continue;
        DPCG_HIP(q);
        if (*prog == v && enq > k) {
            set_error("PCG driver (null space): enqueued updates finished without reporting progress");
            return DPCG_ERR_STATE;
        }
    }
    launch_project(h, h->x, h->x, s);                                                  // the minimum-norm solution
    launch_final_check(h->scal, s);
    DPCG_HIP(hipMemcpyAsync(h->scal_host, h->scal, sizeof(Scalars), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    const auto t1 = std::chrono::steady_clock::now();
    DPCG_TRY(check_spin_errors(h, s));
    const Scalars sc = *h->scal_host;
    if (c.seconds) *c.seconds = std::chrono::duration<double>(t1 - t0).count();
    if (c.iters) *c.iters = sc.k;
    if (c.final_res) *c.final_res = sc.res;
    if (c.res_history) DPCG_HIP(hipMemcpyAsync(c.res_history, h->hist, (size_t)(sc.k + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (c.x) {
        if (h->perm) launch_scatter_f64(n, h->perm, h->x, c.x, s);
        else DPCG_HIP(hipMemcpyAsync(c.x, h->x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (c.res_history) DPCG_HIP(hipStreamSynchronize(s));
    DPCG_CHECK_LAUNCH();
    return sc.status;
}
