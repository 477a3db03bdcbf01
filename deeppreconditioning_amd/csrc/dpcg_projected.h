// PCG with a small block of columns carried through the recurrence: the search direction is p = (z - V c) + beta p with c = U^T z.
//   null space (dpcg_nullspace.hip):  U = V = Z, also t = Z^T r, rho = <r,z> - t^T c
//   deflation  (dpcg_deflation.hip):  U = A W, V = W,            rho = <r,z>
// One kernel per role, written over a basis policy (NullBasis, DeflationBasis below); the host pieces that launch them for either
// family; and the several-sums-at-once reductions they stand on.  Include from .hip files only.  -ffp-contract=off as dpcg_pcg.hip.
//
// Launches per update, M = I / Jacobi -- those of a plain solve in its three-kernel form:
//   K1  the handle's SpMV with its partials of <p,q> (launch_spmv with the iteration head: unchanged)
//   K2  k_proj_update_r:   alpha;  r -= alpha q;  z = dinv r on the fly;  per-workgroup partials of <r,r>, <r,z> and the basis' sums
//   K3  k_proj_update_xp:  those sums re-reduced in one fixed order by every workgroup;  rho', beta;  workgroup 0 records the history
//                          and runs the test;  x += alpha p;  p = (z - V c) + beta p, the columns subtracted in ascending order
// Any other M: K2 with <r,r> only, the handle's apply, k_proj_dots for the other sums, K3.
// All vectors are handle-owned: 16-byte accesses, the next pair requested before the current one is consumed.  No float atomics: wave
// tree, four wave sums in LDS, the partials in a fixed order.  The control words (done, done_seen, k, the progress word) are the
// plain solve's (Scalars, record_and_test); the extra sums live in the attachment's own partial buffer.
#pragma once

#include <chrono>
#include <type_traits>

#include "dpcg_device.h"
#include "dpcg_host.h"

namespace dpcg {

// ---- several sums at once: N running sums per lane -> wave tree -> four wave sums each in LDS -> one fixed-order add, and the
// per-workgroup partials of such sums kept in "slots" of kMaxGrid doubles that every workgroup of a later kernel re-reduces in the
// same order
template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double *sh) {   // sh: 4 N doubles
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int j = 0; j < N; ++j) sh[4 * j + (threadIdx.x >> 6)] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = ((sh[4 * j] + sh[4 * j + 1]) + sh[4 * j + 2]) + sh[4 * j + 3];
}

// slots first .. first + N - 1 of the partial buffer, G partials each, summed as reduce_partials sums them
template <int N>
__device__ __forceinline__ void reduce_slots(const double *__restrict__ part, int first, int G, double (&v)[N], double *sh) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double *__restrict__ pj = part + (int64_t)(first + j) * kMaxGrid;
        double s = 0.0;
        for (int i = threadIdx.x; i < G; i += kBlock) s += pj[i];
        v[j] = s;
    }
    block_sum_n<N>(v, sh);
}

template <int N>
__device__ __forceinline__ void store_slots(double *__restrict__ part, int first, const double (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) part[(int64_t)(first + j) * kMaxGrid + blockIdx.x] = v[j];
}

// partial slots, kMaxGrid doubles each: <r,r> (start: the first tested quantity), <r,z>, the basis' kSums column sums, <b,b>
constexpr int kProjSlotRR = 0, kProjSlotRZ = 1, kProjSlotCols = 2;

// ---- the basis policies: all that differs between the two families ----------------------------------------------------------------
//   K, kSums       coefficients c, and the sums a row adds beyond <r,r> and <r,z>
//   load           rows 2 i, 2 i + 1 of the K columns
//   add_pair/row   a row pair's / one row's terms of the kSums sums (acc: the first of them)
//   sum_entry      column j's entry in a sum;  sub_entry / sub_lane: in the subtraction z - V c (from memory / from a loaded pair)
//   coefficients   from the re-reduced sums v (slot order) to c, returning rho;  first_test: the quantity the start tests
// Which array K2 and K3 read is the host's half of the policy: ProjectedBasis below.

// Z: K orthonormal columns, or (CONST) the one column 1/sqrt(n) that is never read -- zc stands for its entries
template <int KV, bool CONST>
struct NullBasis {
    static constexpr int K = KV, kSums = 2 * KV;       // Z^T z (K of them), Z^T r (K)
    static constexpr bool kConst = CONST;
    static __device__ __forceinline__ void load(const double *__restrict__ Z, int64_t ld, int64_t i, double2 *zv) {
        if (CONST) return;
#pragma unroll
        for (int j = 0; j < K; ++j) zv[j] = reinterpret_cast<const double2 *>(Z + (int64_t)j * ld)[i];
    }
    static __device__ __forceinline__ void add_pair(double *acc, const double2 *zc, const double2 &zn, const double2 &rn) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (CONST) {
                acc[j] += zn.x;
                acc[j] += zn.y;
                acc[K + j] += rn.x;
                acc[K + j] += rn.y;
            } else {
                acc[j] += zc[j].x * zn.x;
                acc[j] += zc[j].y * zn.y;
                acc[K + j] += zc[j].x * rn.x;
                acc[K + j] += zc[j].y * rn.y;
            }
        }
    }
    static __device__ __forceinline__ void add_row(double *acc, const double *__restrict__ Z, int64_t ld, int64_t i, double zn, double rn) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double zj = CONST ? 1.0 : Z[(int64_t)j * ld + i];
            acc[j] += zj * zn;
            acc[K + j] += zj * rn;
        }
    }
    static __device__ __forceinline__ double sum_entry(const double *__restrict__ Z, int64_t ld, int j, int64_t i) {
        return CONST ? 1.0 : Z[(int64_t)j * ld + i];
    }
    static __device__ __forceinline__ double sub_entry(const double *__restrict__ Z, int64_t ld, int j, int64_t i, double zc) {
        return CONST ? zc : Z[(int64_t)j * ld + i];
    }
    static __device__ __forceinline__ double sub_lane(double stored, double zc) { return CONST ? zc : stored; }
    // Z^T z and Z^T r scaled to the orthonormal Z (CONST: the plain sums times 1/sqrt(n)), t^T s in column order;  rho = <r, P z>
    template <int N>
    static __device__ __forceinline__ double coefficients(const double (&v)[N], double (&s)[K], double zc) {
        double t[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            s[j] = v[kProjSlotCols + j];
            t[j] = v[kProjSlotCols + K + j];
        }
        double ts = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (CONST) {
                s[j] = zc * s[j];
                t[j] = zc * t[j];
            }
            ts += t[j] * s[j];
        }
        return v[kProjSlotRZ] - ts;
    }
    // <p,p> = <z,z> - s^T s (the preconditioned residual the recurrence starts from), or <r,r>
    static __device__ __forceinline__ double first_test(double tt, const double (&s)[K], int init_check_r) {
        if (!init_check_r) {
#pragma unroll
            for (int j = 0; j < K; ++j) tt = tt - s[j] * s[j];
        }
        return tt;
    }
};

// W with W^T A W = I and A W beside it, KV = 1, 2, 4 or 8 columns stored (the extra ones zero: mu_j = 0 exactly, z - 0 * 0 = z exactly)
template <int KV>
struct DeflationBasis {
    static constexpr int K = KV, kSums = KV;           // mu = AW^T z
    static __device__ __forceinline__ void load(const double *__restrict__ W, int64_t ld, int64_t i, double2 *wv) {
#pragma unroll
        for (int j = 0; j < K; ++j) wv[j] = reinterpret_cast<const double2 *>(W + (int64_t)j * ld)[i];
    }
    static __device__ __forceinline__ void add_pair(double *acc, const double2 *wc, const double2 &zn, const double2 &) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            acc[j] += wc[j].x * zn.x;
            acc[j] += wc[j].y * zn.y;
        }
    }
    static __device__ __forceinline__ void add_row(double *acc, const double *__restrict__ AW, int64_t ld, int64_t i, double zn, double) {
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += AW[(int64_t)j * ld + i] * zn;
    }
    static __device__ __forceinline__ double sum_entry(const double *__restrict__ W, int64_t ld, int j, int64_t i) { return W[(int64_t)j * ld + i]; }
    static __device__ __forceinline__ double sub_entry(const double *__restrict__ W, int64_t ld, int j, int64_t i, double) {
        return W[(int64_t)j * ld + i];
    }
    static __device__ __forceinline__ double sub_lane(double stored, double) { return stored; }
    template <int N>
    static __device__ __forceinline__ double coefficients(const double (&v)[N], double (&mu)[K], double) {
#pragma unroll
        for (int j = 0; j < K; ++j) mu[j] = v[kProjSlotCols + j];
        return v[kProjSlotRZ];
    }
    static __device__ __forceinline__ double first_test(double tt, const double (&)[K], int) { return tt; }
};

namespace {

// K2.  PRE: 0 = M = I (z = r), 1 = Jacobi (z = dinv r, not stored: K3 forms the same product again), 2 = any other M (only
// r -= alpha q and <r,r>: the apply and k_proj_dots follow).
template <class B, int PRE>
__global__ __launch_bounds__(kBlock) void k_proj_update_r(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part_pq,
                                                          int n_part_pq, const double *__restrict__ q, double *__restrict__ r,
                                                          const double *__restrict__ dinv, const double *__restrict__ cols, int64_t ld,
                                                          double *__restrict__ part) {
    constexpr int K = B::K;
    constexpr int N = PRE == 2 ? 1 : 2 + B::kSums;
    constexpr int KL = PRE == 2 ? 1 : K;                                // (no column is read when the apply follows)
    __shared__ double sh[4 * N > 8 ? 4 * N : 8];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ q2 = reinterpret_cast<const double2 *>(q);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ r2 = reinterpret_cast<double2 *>(r);
    double2 qa = make_double2(0, 0), ra = qa, da = qa, ca[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) ca[j] = qa;
    bool have = i < n2;
    if (have) {
        qa = q2[i];
        ra = r2[i];
        if (PRE == 1) da = d2[i];
        if constexpr (PRE != 2) B::load(cols, ld, i, ca);
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
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;         // read by K3 (a later kernel)
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    while (have) {
        const int64_t cur = i;
        const double2 qc = qa, rc = ra, dc = da;
        double2 cc[KL];
#pragma unroll
        for (int j = 0; j < KL; ++j) cc[j] = ca[j];
        i += stride;
        have = i < n2;
        if (have) {
            qa = q2[i];
            ra = r2[i];
            if (PRE == 1) da = d2[i];
            if constexpr (PRE != 2) B::load(cols, ld, i, ca);
        }
        double2 rn;
        rn.x = rc.x - alpha * qc.x;
        rn.y = rc.y - alpha * qc.y;
        r2[cur] = rn;
        acc[kProjSlotRR] += rn.x * rn.x;
        acc[kProjSlotRR] += rn.y * rn.y;
        if constexpr (PRE != 2) {
            double2 zn = rn;
            if (PRE == 1) {
                zn.x = dc.x * rn.x;
                zn.y = dc.y * rn.y;
            }
            acc[kProjSlotRZ] += rn.x * zn.x;
            acc[kProjSlotRZ] += rn.y * zn.y;
            B::add_pair(acc + kProjSlotCols, cc, zn, rn);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {               // odd tail element
        const int64_t e = n - 1;
        const double rn = r[e] - alpha * q[e];
        r[e] = rn;
        acc[kProjSlotRR] += rn * rn;
        if constexpr (PRE != 2) {
            const double zn = PRE == 1 ? dinv[e] * rn : rn;
            acc[kProjSlotRZ] += rn * zn;
            B::add_row(acc + kProjSlotCols, cols, ld, e, zn, rn);
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) store_slots<N>(part, 0, acc);
}

// Partials of <r,z> and the basis' sums for a z that lies in memory (any M in the loop; the start of every solve).  init: also the
// first tested quantity -- <r,r> (init_check_r) or <z,z>, which B::first_test completes -- and <b,b>.  sc (loop only): skipped once
// the solve is done.
template <class B>
__global__ __launch_bounds__(kBlock) void k_proj_dots(int64_t n, const Scalars *__restrict__ sc, const double *__restrict__ r,
                                                      const double *__restrict__ z, const double *__restrict__ b,
                                                      const double *__restrict__ cols, int64_t ld, double *__restrict__ part, int init,
                                                      int init_check_r) {
    constexpr int kBB = 2 + B::kSums;             // [0] first test, [1] <r,z>, the column sums, [kBB] <b,b>
    constexpr int N = kBB + 1;
    __shared__ double sh[4 * N];
    if (sc && sc->done) return;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ri = r[i], zi = z[i];
        acc[kProjSlotRZ] += ri * zi;
        B::add_row(acc + kProjSlotCols, cols, ld, i, zi, ri);
        if (init) {
            const double bi = b[i];
            acc[kProjSlotRR] += init_check_r ? ri * ri : zi * zi;
            acc[kBB] += bi * bi;
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < kBB; ++j) part[(int64_t)j * kMaxGrid + blockIdx.x] = acc[j];
        if (init) {
            part[(int64_t)kProjSlotRR * kMaxGrid + blockIdx.x] = acc[kProjSlotRR];
            part[(int64_t)kBB * kMaxGrid + blockIdx.x] = acc[kBB];
        }
    }
}

// Start of a solve: every workgroup re-reduces what k_proj_dots (init) left; p = z - V c; workgroup 0 sets up the control words and
// runs the first test.
template <class B>
__global__ __launch_bounds__(kBlock) void k_proj_init(int64_t n, Scalars *sc, const double *__restrict__ part, int G,
                                                      const double *__restrict__ z, double *__restrict__ p,
                                                      const double *__restrict__ cols, int64_t ld, double zc, double rtol_sq,
                                                      double atol_sq, double *hist, int hist_cap, unsigned long long *progress,
                                                      int init_check_r) {
    constexpr int K = B::K;
    constexpr int N = 3 + B::kSums;
    __shared__ double sh[4 * N];
    double v[N], c[K];
    reduce_slots<N>(part, 0, G, v, sh);
    const double rho = B::coefficients(v, c, zc);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double pi = z[i];
#pragma unroll
        for (int j = 0; j < K; ++j) pi = pi - B::sub_entry(cols, ld, j, i, zc) * c[j];
        p[i] = pi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double tt = B::first_test(v[kProjSlotRR], c, init_check_r);
        sc->bb = v[2 + B::kSums];
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

// K3.  zsrc: r for PRE 0 and 1 (Jacobi: times dinv, the product K2 summed), the stored z for PRE 2.
template <class B, int PRE>
__global__ __launch_bounds__(kBlock) void k_proj_update_xp(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part, int G,
                                                           const double *__restrict__ zsrc, const double *__restrict__ dinv,
                                                           double *__restrict__ p, double *__restrict__ x,
                                                           const double *__restrict__ cols, int64_t ld, double zc,
                                                           double *__restrict__ hist, int hist_cap) {
    constexpr int K = B::K;
    constexpr int N = 2 + B::kSums;
    __shared__ double sh[4 * N];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ z2 = reinterpret_cast<const double2 *>(zsrc);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ p2 = reinterpret_cast<double2 *>(p);
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    double2 ta = make_double2(0, 0), pa = ta, xa = ta, da = ta, ca[K];
#pragma unroll
    for (int j = 0; j < K; ++j) ca[j] = ta;
    bool have = i < n2;
    if (have) {
        ta = z2[i];
        pa = p2[i];
        xa = x2[i];
        if (PRE == 1) da = d2[i];
        B::load(cols, ld, i, ca);
    }
    // `done_seen`, not `done` (see k_update_xp): workgroup 0 of THIS launch sets `done`
    const int done_seen = sc->done_seen;
    double rz_old = sc->rz, alpha = sc->alpha;
    pin_scalar(rz_old);
    pin_scalar(alpha);
    if (done_seen) return;
    double v[N], c[K];
    reduce_slots<N>(part, 0, G, v, sh);
    const double rz_new = B::coefficients(v, c, zc);
    const double beta = rz_new / rz_old;
    if (blockIdx.x == 0 && threadIdx.x == 0) record_and_test(sc, v[kProjSlotRR], rz_new, hist, hist_cap, sc->k + 1);
    while (have) {
        const int64_t cur = i;
        double2 tc = ta;
        const double2 pc = pa, xc = xa, dc = da;
        double2 cv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) cv[j] = ca[j];
        i += stride;
        have = i < n2;
        if (have) {
            ta = z2[i];
            pa = p2[i];
            xa = x2[i];
            if (PRE == 1) da = d2[i];
            B::load(cols, ld, i, ca);
        }
        if (PRE == 1) {                                                 // z = dinv r, recomputed
            tc.x = dc.x * tc.x;
            tc.y = dc.y * tc.y;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {                                   // z - V c, columns ascending
            tc.x = tc.x - B::sub_lane(cv[j].x, zc) * c[j];
            tc.y = tc.y - B::sub_lane(cv[j].y, zc) * c[j];
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
        for (int j = 0; j < K; ++j) te = te - B::sub_entry(cols, ld, j, e, zc) * c[j];
        p[e] = te + beta * pe;
    }
}

// partials of (columns)^T v into slots kProjSlotCols .. + K
template <class B>
__global__ __launch_bounds__(kBlock) void k_proj_col_dots(int64_t n, const double *__restrict__ v, const double *__restrict__ cols,
                                                          int64_t ld, double *__restrict__ part) {
    constexpr int K = B::K;
    __shared__ double sh[4 * K];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double vi = v[i];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += B::sum_entry(cols, ld, j, i) * vi;
    }
    block_sum_n<K>(acc, sh);
    if (threadIdx.x == 0) store_slots<K>(part, kProjSlotCols, acc);
}

// ---- the host's half -----------------------------------------------------------------------------------------------------------------
// What an attachment hands the kernels.  A family (NullFamily, DeflationFamily) turns `shape` into a basis type:
// Family::with_shape(shape, f) calls f(B{}) for the one B that serves it.
struct ProjectedBasis {
    int shape;
    const double *k2_cols, *k3_cols;     // the columns K2 sums against (U), the ones K3 and the start subtract (V)
    int64_t ld;                          // rows between two columns
    double zc;                           // NullBasis<1, true>'s entry; unused otherwise
    double *part;                        // (3 + kSums) x kMaxGrid
};

// (shape, pre) as compile-time constants: f(B{}, std::integral_constant<int, PRE>{})
template <class Family, class F>
void projected_dispatch(int shape, int pre, F &&f) {
    Family::with_shape(shape, [&](auto basis) {
        if (pre == 0) f(basis, std::integral_constant<int, 0>{});
        else if (pre == 1) f(basis, std::integral_constant<int, 1>{});
        else f(basis, std::integral_constant<int, 2>{});
    });
}

template <class Family>
void launch_projected_col_dots(const dpcg_system *h, const ProjectedBasis &pb, const double *v, const double *cols, hipStream_t s) {
    Family::with_shape(pb.shape, [&](auto basis) {
        hipLaunchKernelGGL((k_proj_col_dots<decltype(basis)>), dim3(h->vec_grid), dim3(kBlock), 0, s, h->A.n, v, cols, pb.ld, pb.part);
    });
}

template <class Family>
void launch_projected_dots(const dpcg_system *h, const ProjectedBasis &pb, const Scalars *sc, const double *r, const double *z,
                           const double *b, bool init, int init_check_r, hipStream_t s) {
    Family::with_shape(pb.shape, [&](auto basis) {
        hipLaunchKernelGGL((k_proj_dots<decltype(basis)>), dim3(h->vec_grid), dim3(kBlock), 0, s, h->A.n, sc, r, z, b, pb.k2_cols, pb.ld,
                           pb.part, init ? 1 : 0, init_check_r);
    });
}

// one update as launches on s
template <class Family>
int enqueue_projected_update(dpcg_system *h, const ProjectedBasis &pb, hipStream_t s) {
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    const int pre = precond_class(h);
    IterCtl ctl{h->scal};
    launch_spmv(h->A, h->planA, h->p, h->q, h->part_pq, &ctl, s);                                // K1
    projected_dispatch<Family>(pb.shape, pre, [&](auto basis, auto pre_c) {                       // K2
        hipLaunchKernelGGL((k_proj_update_r<decltype(basis), decltype(pre_c)::value>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq,
                           h->planA.grid, h->q, h->r, h->dinv, pb.k2_cols, pb.ld, pb.part);
    });
    if (pre == 2) {
        DPCG_TRY(apply_precond(h, h->r, h->z, s, true));
        launch_projected_dots<Family>(h, pb, h->scal, h->r, h->z, nullptr, false, 0, s);
    }
    projected_dispatch<Family>(pb.shape, pre, [&](auto basis, auto pre_c) {                       // K3
        hipLaunchKernelGGL((k_proj_update_xp<decltype(basis), decltype(pre_c)::value>), dim3(G), dim3(kBlock), 0, s, n, h->scal, pb.part, G,
                           pre == 2 ? h->z : h->r, h->dinv, h->p, h->x, pb.k3_cols, pb.ld, pb.zc, h->hist, h->hist_cap);
    });
    return DPCG_OK;
}

// The start of a solve once r stands (b: the right-hand side r was formed against, in the handle's numbering): z = M r, the init
// sums, the first direction and the control words; the timer starts when that has drained.
template <class Family>
int start_projected(dpcg_system *h, const ProjectedBasis &pb, const double *b, const SolveCall &c,
                    std::chrono::steady_clock::time_point *t0) {
    hipStream_t s = c.s;
    const double *z = h->precond == DPCG_PRECOND_NONE ? h->r : h->z;
    if (h->precond != DPCG_PRECOND_NONE) DPCG_TRY(apply_precond(h, h->r, h->z, s));
    const int init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    launch_projected_dots<Family>(h, pb, nullptr, h->r, z, b, true, init_check_r, s);
    Family::with_shape(pb.shape, [&](auto basis) {
        hipLaunchKernelGGL((k_proj_init<decltype(basis)>), dim3(h->vec_grid), dim3(kBlock), 0, s, h->A.n, h->scal, pb.part, h->vec_grid, z,
                           h->p, pb.k3_cols, pb.ld, pb.zc, c.rtol_sq, c.atol_sq, h->hist, h->hist_cap, extras()[h].prog_dev, init_check_r);
    });
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    *t0 = std::chrono::steady_clock::now();
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg
