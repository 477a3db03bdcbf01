// Deflated PCG (dpcg_set_deflation / dpcg_get_deflation, include/dpcg.h): Saad, Yeung, Erhel, Guyomarc'h, "A deflated version of the
// conjugate gradient algorithm", SISC 21 (2000); with piecewise-constant vectors it is Nicolaides' subdomain deflation.  Not in the
// reference.  Compiled with -ffp-contract=off like dpcg_pcg.hip and dpcg_nullspace.hip.
//
// W is n x k (1 <= k <= 8) with W^T A W = I, AW = A W stored beside it.  The solve (the contract is in include/dpcg.h):
//     start:   r = b - A x0 (x0 NULL: r = b);  c = W^T r;  x = x0 + W c;  r = r - AW c;  z = M r;  mu = AW^T z;  p = z - W mu;  rho = <r,z>
//     update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  z = M r;  mu = AW^T z;  rho' = <r,z>;
//              p = (z - W mu) + (rho'/rho) p
// Launches per update, M = I / Jacobi -- those of a plain solve in its three-kernel form:
//   K1    the handle's SpMV with its partials of <p,q> (launch_spmv with the iteration head: unchanged)
//   K2d   k_df_update_r:   alpha;  r -= alpha q;  z = dinv r on the fly;  per-workgroup partials of <r,r>, <r,z>, AW^T z
//   K3d   k_df_update_xp:  the 2 + k sums re-reduced in one fixed order by every workgroup;  beta;  workgroup 0 records the history
//                          and runs the test;  x += alpha p;  p = (z - W mu) + beta p, the columns subtracted in ascending order
// Any other M: K2d with <r,r> only, the handle's apply, k_df_dots for the other 1 + k sums, K3d.
// K2d reads AW and K3d reads W: 8 k bytes per row each on top of the 40 a Jacobi update moves per pass.  The kernels exist for
// 1, 2, 4 and 8 columns; W and AW are stored with that many, the extra columns zero (mu_j = 0 exactly, z - 0 * 0 = z exactly).
// Columns are ld rows apart, ld = n rounded up to a multiple of 1024 (the layout dpcg_guess.hip's CholQR2 kernels run on, which the
// attach shares), the padding rows zero.  16-byte accesses, the next pair requested before the current one is consumed.  No float
// atomics: wave tree, four wave sums in LDS, the partials in a fixed order.  The control words (Scalars, record_and_test) are the
// plain solve's; the extra sums live in the deflation's own partial buffer.
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_slots.h"

namespace dpcg {

constexpr int kDfMaxK = 8;
constexpr int64_t kDfSpan = 1024;             // ld is a multiple of it (dpcg_guess.hip's kernels take whole workgroups of 512 rows)
constexpr double kDfTolDep = 1e-7;            // a column is dependent when its pivot is <= kDfTolDep^2 G_jj (the guess's default)
// partial slots, kMaxGrid doubles each: <r,r> (start: the first tested quantity), <r,z>, AW^T z or W^T r (K of them), <b,b>
constexpr int kDfSlotRR = 0, kDfSlotRZ = 1, kDfSlotMu = 2;
constexpr int kDfSlots = 3 + kDfMaxK;
constexpr int kDfCoefGram = 0, kDfCoefRinv = kDfMaxK * kDfMaxK, kDfCoefCount = 2 * kDfMaxK * kDfMaxK;

struct Deflation {
    int k = 0;                      // columns attached
    int kp = 0;                     // columns stored: 1, 2, 4 or 8
    int64_t ld = 0;
    double *W = nullptr;            // device, kp columns in the HANDLE's numbering, W^T A W = I
    double *AW = nullptr;           // A W, the same layout
    double *part = nullptr;         // kDfSlots x kMaxGrid
    double *gs_part = nullptr;      // CholQR2: k x ld / 128 wave partials
    double *coef = nullptr;         // CholQR2: the Gram matrix and R^-1
};

namespace {

// rows 2 i, 2 i + 1 of the K columns
template <int K>
__device__ __forceinline__ void w_load(const double *__restrict__ W, int64_t ld, int64_t i, double2 (&wv)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) wv[j] = reinterpret_cast<const double2 *>(W + (int64_t)j * ld)[i];
}

// K2d.  PRE: 0 = M = I (z = r), 1 = Jacobi (z = dinv r, not stored: K3d forms the same product again), 2 = any other M (only
// r -= alpha q and <r,r>: the apply and k_df_dots follow).
template <int K, int PRE>
__global__ __launch_bounds__(kBlock) void k_df_update_r(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part_pq,
                                                        int n_part_pq, const double *__restrict__ q, double *__restrict__ r,
                                                        const double *__restrict__ dinv, const double *__restrict__ AW, int64_t ld,
                                                        double *__restrict__ part) {
    constexpr int N = PRE == 2 ? 1 : 2 + K;
    constexpr int KL = PRE == 2 ? 1 : K;                                // (no column is read when the apply follows)
    __shared__ double sh[4 * N > 8 ? 4 * N : 8];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ q2 = reinterpret_cast<const double2 *>(q);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ r2 = reinterpret_cast<double2 *>(r);
    double2 qa = make_double2(0, 0), ra = qa, da = qa, wa[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) wa[j] = qa;
    bool have = i < n2;
    if (have) {
        qa = q2[i];
        ra = r2[i];
        if (PRE == 1) da = d2[i];
        if constexpr (PRE != 2) w_load<K>(AW, ld, i, wa);
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
    if (blockIdx.x == 0 && threadIdx.x == 0) sc->alpha = alpha;         // read by K3d (a later kernel)
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    while (have) {
        const int64_t cur = i;
        const double2 qc = qa, rc = ra, dc = da;
        double2 wc[KL];
#pragma unroll
        for (int j = 0; j < KL; ++j) wc[j] = wa[j];
        i += stride;
        have = i < n2;
        if (have) {
            qa = q2[i];
            ra = r2[i];
            if (PRE == 1) da = d2[i];
            if constexpr (PRE != 2) w_load<K>(AW, ld, i, wa);
        }
        double2 rn;
        rn.x = rc.x - alpha * qc.x;
        rn.y = rc.y - alpha * qc.y;
        r2[cur] = rn;
        acc[kDfSlotRR] += rn.x * rn.x;
        acc[kDfSlotRR] += rn.y * rn.y;
        if constexpr (PRE != 2) {
            double2 zn = rn;
            if (PRE == 1) {
                zn.x = dc.x * rn.x;
                zn.y = dc.y * rn.y;
            }
            acc[kDfSlotRZ] += rn.x * zn.x;
            acc[kDfSlotRZ] += rn.y * zn.y;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc[kDfSlotMu + j] += wc[j].x * zn.x;
                acc[kDfSlotMu + j] += wc[j].y * zn.y;
            }
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {               // odd tail element
        const int64_t e = n - 1;
        const double rn = r[e] - alpha * q[e];
        r[e] = rn;
        acc[kDfSlotRR] += rn * rn;
        if constexpr (PRE != 2) {
            const double zn = PRE == 1 ? dinv[e] * rn : rn;
            acc[kDfSlotRZ] += rn * zn;
#pragma unroll
            for (int j = 0; j < K; ++j) acc[kDfSlotMu + j] += AW[(int64_t)j * ld + e] * zn;
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) store_slots<N>(part, 0, acc);
}

// Partials of <r,z> and AW^T z for a z that lies in memory (any M in the loop; the start of every solve).  init: also the first
// tested quantity -- <r,r> (init_check_r) or <z,z> -- and <b,b>.  sc (loop only): skipped once the solve is done.
template <int K>
__global__ __launch_bounds__(kBlock) void k_df_dots(int64_t n, const Scalars *__restrict__ sc, const double *__restrict__ r,
                                                    const double *__restrict__ z, const double *__restrict__ b,
                                                    const double *__restrict__ AW, int64_t ld, double *__restrict__ part, int init,
                                                    int init_check_r) {
    constexpr int N = 3 + K;                      // [0] first test, [1] <r,z>, mu, [2 + K] <b,b>
    __shared__ double sh[4 * N];
    if (sc && sc->done) return;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ri = r[i], zi = z[i];
        acc[kDfSlotRZ] += ri * zi;
#pragma unroll
        for (int j = 0; j < K; ++j) acc[kDfSlotMu + j] += AW[(int64_t)j * ld + i] * zi;
        if (init) {
            const double bi = b[i];
            acc[kDfSlotRR] += init_check_r ? ri * ri : zi * zi;
            acc[2 + K] += bi * bi;
        }
    }
    block_sum_n<N>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < 2 + K; ++j) part[(int64_t)j * kMaxGrid + blockIdx.x] = acc[j];
        if (init) {
            part[(int64_t)kDfSlotRR * kMaxGrid + blockIdx.x] = acc[kDfSlotRR];
            part[(int64_t)(2 + K) * kMaxGrid + blockIdx.x] = acc[2 + K];
        }
    }
}

// Start of a solve, after the correction: every workgroup re-reduces what k_df_dots (init) left; p = z - W mu; workgroup 0 sets up
// the control words and runs the first test.
template <int K>
__global__ __launch_bounds__(kBlock) void k_df_init(int64_t n, Scalars *sc, const double *__restrict__ part, int G,
                                                    const double *__restrict__ z, double *__restrict__ p,
                                                    const double *__restrict__ W, int64_t ld, double rtol_sq, double atol_sq,
                                                    double *hist, int hist_cap, unsigned long long *progress) {
    constexpr int N = 3 + K;
    __shared__ double sh[4 * N];
    double v[N];
    reduce_slots<N>(part, 0, G, v, sh);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double pi = z[i];
#pragma unroll
        for (int j = 0; j < K; ++j) pi = pi - W[(int64_t)j * ld + i] * v[kDfSlotMu + j];
        p[i] = pi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc->bb = v[2 + K];
        sc->rz = v[kDfSlotRZ];
        sc->alpha = 0.0;
        sc->rtol_sq = rtol_sq;
        sc->atol_sq = atol_sq;
        sc->done = 0;
        sc->status = DPCG_MAX_ITER;
        sc->done_seen = 0;
        sc->progress = progress;
        record_and_test(sc, v[kDfSlotRR], v[kDfSlotRZ], hist, hist_cap, 0);
    }
}

// K3d.  zsrc: r for PRE 0 and 1 (Jacobi: times dinv, the product K2d summed), the stored z for PRE 2.
template <int K, int PRE>
__global__ __launch_bounds__(kBlock) void k_df_update_xp(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part, int G,
                                                         const double *__restrict__ zsrc, const double *__restrict__ dinv,
                                                         double *__restrict__ p, double *__restrict__ x,
                                                         const double *__restrict__ W, int64_t ld, double *__restrict__ hist,
                                                         int hist_cap) {
    constexpr int N = 2 + K;
    __shared__ double sh[4 * N];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ z2 = reinterpret_cast<const double2 *>(zsrc);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ p2 = reinterpret_cast<double2 *>(p);
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    double2 ta = make_double2(0, 0), pa = ta, xa = ta, da = ta, wa[K];
#pragma unroll
    for (int j = 0; j < K; ++j) wa[j] = ta;
    bool have = i < n2;
    if (have) {
        ta = z2[i];
        pa = p2[i];
        xa = x2[i];
        if (PRE == 1) da = d2[i];
        w_load<K>(W, ld, i, wa);
    }
    // `done_seen`, not `done` (see k_update_xp): workgroup 0 of THIS launch sets `done`
    const int done_seen = sc->done_seen;
    double rz_old = sc->rz, alpha = sc->alpha;
    pin_scalar(rz_old);
    pin_scalar(alpha);
    if (done_seen) return;
    double v[N];
    reduce_slots<N>(part, 0, G, v, sh);
    const double rz_new = v[kDfSlotRZ];
    const double beta = rz_new / rz_old;
    if (blockIdx.x == 0 && threadIdx.x == 0) record_and_test(sc, v[kDfSlotRR], rz_new, hist, hist_cap, sc->k + 1);
    while (have) {
        const int64_t cur = i;
        double2 tc = ta;
        const double2 pc = pa, xc = xa, dc = da;
        double2 wv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wv[j] = wa[j];
        i += stride;
        have = i < n2;
        if (have) {
            ta = z2[i];
            pa = p2[i];
            xa = x2[i];
            if (PRE == 1) da = d2[i];
            w_load<K>(W, ld, i, wa);
        }
        if (PRE == 1) {                                                 // z = dinv r, recomputed
            tc.x = dc.x * tc.x;
            tc.y = dc.y * tc.y;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {                                   // z - W mu, columns ascending
            tc.x = tc.x - wv[j].x * v[kDfSlotMu + j];
            tc.y = tc.y - wv[j].y * v[kDfSlotMu + j];
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
        for (int j = 0; j < K; ++j) te = te - W[(int64_t)j * ld + e] * v[kDfSlotMu + j];
        p[e] = te + beta * pe;
    }
}

// The start correction, a kernel pair.  First: partials of c = W^T r into slots kDfSlotMu .. + K
template <int K>
__global__ __launch_bounds__(kBlock) void k_df_wt_dots(int64_t n, const double *__restrict__ r, const double *__restrict__ W, int64_t ld,
                                                       double *__restrict__ part) {
    __shared__ double sh[4 * K];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ri = r[i];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += W[(int64_t)j * ld + i] * ri;
    }
    block_sum_n<K>(acc, sh);
    if (threadIdx.x == 0) store_slots<K>(part, kDfSlotMu, acc);
}

// ... then x += W c and r -= AW c from those partials, the columns in ascending order
template <int K>
__global__ __launch_bounds__(kBlock) void k_df_correct(int64_t n, double *__restrict__ x, double *__restrict__ r,
                                                       const double *__restrict__ W, const double *__restrict__ AW, int64_t ld,
                                                       const double *__restrict__ part, int G) {
    __shared__ double sh[4 * K];
    double c[K];
    reduce_slots<K>(part, kDfSlotMu, G, c, sh);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double xi = x[i], ri = r[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            xi = xi + W[(int64_t)j * ld + i] * c[j];
            ri = ri - AW[(int64_t)j * ld + i] * c[j];
        }
        x[i] = xi;
        r[i] = ri;
    }
}

// one kernel variant per stored width
#define DPCG_DF_SHAPES(df, LAUNCH)             \
    do {                                       \
        if ((df)->kp == 1) { LAUNCH(1); }      \
        else if ((df)->kp == 2) { LAUNCH(2); } \
        else if ((df)->kp == 4) { LAUNCH(4); } \
        else { LAUNCH(8); }                    \
    } while (0)

inline int df_pre(const dpcg_system *h) { return h->precond == DPCG_PRECOND_NONE ? 0 : (h->precond == DPCG_PRECOND_JACOBI ? 1 : 2); }

void launch_df_dots(const dpcg_system *h, const Scalars *sc, const double *r, const double *z, const double *b, bool init, int init_check_r,
                    hipStream_t s) {
    const Deflation *df = h->df;
#define DPCG_DF_L(KV)                                                                                                                 \
    hipLaunchKernelGGL((k_df_dots<KV>), dim3(h->vec_grid), dim3(kBlock), 0, s, h->A.n, sc, r, z, b, df->AW, df->ld, df->part, init ? 1 : 0, \
                       init_check_r)
    DPCG_DF_SHAPES(df, DPCG_DF_L);
#undef DPCG_DF_L
}

// one update as launches on s
int enqueue_df_update(dpcg_system *h, hipStream_t s) {
    const Deflation *df = h->df;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    const int pre = df_pre(h);
    IterCtl ctl{h->scal};
    launch_spmv(h->A, h->planA, h->p, h->q, h->part_pq, &ctl, s);                                // K1
#define DPCG_DF_K2(KV)                                                                                                         \
    do {                                                                                                                       \
        if (pre == 0)                                                                                                          \
            hipLaunchKernelGGL((k_df_update_r<KV, 0>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, df->AW, df->ld, df->part);                                                       \
        else if (pre == 1)                                                                                                     \
            hipLaunchKernelGGL((k_df_update_r<KV, 1>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, df->AW, df->ld, df->part);                                                       \
        else                                                                                                                   \
            hipLaunchKernelGGL((k_df_update_r<KV, 2>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, h->planA.grid, h->q, \
                               h->r, h->dinv, df->AW, df->ld, df->part);                                                       \
    } while (0)
    DPCG_DF_SHAPES(df, DPCG_DF_K2);                                                               // K2d
#undef DPCG_DF_K2
    if (pre == 2) {
        DPCG_TRY(apply_precond(h, h->r, h->z, s, true));
        launch_df_dots(h, h->scal, h->r, h->z, nullptr, false, 0, s);
    }
#define DPCG_DF_K3(KV)                                                                                                           \
    do {                                                                                                                         \
        if (pre == 0)                                                                                                            \
            hipLaunchKernelGGL((k_df_update_xp<KV, 0>), dim3(G), dim3(kBlock), 0, s, n, h->scal, df->part, G, h->r, h->dinv, h->p, \
                               h->x, df->W, df->ld, h->hist, h->hist_cap);                                                       \
        else if (pre == 1)                                                                                                       \
            hipLaunchKernelGGL((k_df_update_xp<KV, 1>), dim3(G), dim3(kBlock), 0, s, n, h->scal, df->part, G, h->r, h->dinv, h->p, \
                               h->x, df->W, df->ld, h->hist, h->hist_cap);                                                       \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_df_update_xp<KV, 2>), dim3(G), dim3(kBlock), 0, s, n, h->scal, df->part, G, h->z, h->dinv, h->p, \
                               h->x, df->W, df->ld, h->hist, h->hist_cap);                                                       \
    } while (0)
    DPCG_DF_SHAPES(df, DPCG_DF_K3);                                                               // K3d
#undef DPCG_DF_K3
    return DPCG_OK;
}

void release(Deflation *df) {
    if (!df) return;
    dev_free(df->W);
    dev_free(df->AW);
    dev_free(df->part);
    dev_free(df->gs_part);
    dev_free(df->coef);
    delete df;
}

// AW = A W by k calls of the handle's SpMV, then CholQR2 in the A inner product, as dpcg_guess.hip does after new values (its device
// pieces): twice G = W^T AW on the device, G = R^T R on the host, W <- W R^-1 and AW <- AW R^-1 in place.  A dependent column -- a
// pivot <= kDfTolDep^2 G_jj -- is refused (`who` names the caller in the text), not dropped.
int a_orthonormalise(dpcg_system *h, Deflation *df, const char *who, hipStream_t s) {
    const int k = df->k;
    DPCG_TRY(ensure_work(h, 0, false, false));
    for (int j = 0; j < k; ++j) launch_spmv(h->A, h->planA, df->W + (int64_t)j * df->ld, df->AW + (int64_t)j * df->ld, nullptr, nullptr, s);
    DPCG_CHECK_LAUNCH();
    std::vector<double> G((size_t)k * k), T;
    for (int round = 0; round < 2; ++round) {
        // column j of the Gram matrix: G[i][j] = <w_i, AW_j>, kept at G[j * k + i]
        for (int j = 0; j < k; ++j)
            gs_gram_column(df->ld, k, df->W, df->AW + (int64_t)j * df->ld, df->gs_part, df->coef + kDfCoefGram + j * k, s);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipMemcpyAsync(G.data(), df->coef + kDfCoefGram, (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        const int keep = gs_cholesky_rinv(G, k, kDfTolDep * kDfTolDep, T);
        if (keep < k) {
            char buf[320];
            snprintf(buf, sizeof(buf), "%s: column %d of W depends on the columns before it in the A inner product (or is zero, or A is not "
                     "positive definite on it): its pivot is <= tol^2 G_jj = %.3e (tol = %.1e)", who, keep,
                     kDfTolDep * kDfTolDep * G[(size_t)keep * k + keep], kDfTolDep);
            set_error(buf);
            return DPCG_ERR_INVALID;
        }
        DPCG_HIP(hipMemcpyAsync(df->coef + kDfCoefRinv, T.data(), (size_t)k * k * sizeof(double), hipMemcpyHostToDevice, s));
        gs_rmul_pair(df->ld, k, df->W, df->AW, df->coef + kDfCoefRinv, s);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipStreamSynchronize(s));      // (T is overwritten by the next round)
    }
    return DPCG_OK;
}

int read_perm(const dpcg_system *h, std::vector<int32_t> &perm, hipStream_t s) {
    perm.clear();
    if (!h->perm) return DPCG_OK;
    perm.resize((size_t)h->A.n);
    DPCG_HIP(hipMemcpyAsync(perm.data(), h->perm, perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

void free_deflation(dpcg_system *h) {
    release(h->df);
    h->df = nullptr;
}

const char *deflation_refusal(const dpcg_system *h, int flags, const double *x_true) {
    if (!h->df) return nullptr;
    if (flags & DPCG_SINGLE_REDUCTION) return "dpcg_solve: DPCG_SINGLE_REDUCTION is not available on a handle with a deflation (the deflated recurrence is the standard one)";
    if (flags & DPCG_SPMV_F32) return "dpcg_solve: DPCG_SPMV_F32 is not available on a handle with a deflation";
    if (flags & DPCG_TEAM) return "dpcg_solve: DPCG_TEAM is not available on a handle with a deflation (no one-launch form deflates)";
    if (x_true) return "dpcg_solve: x_true tracking is not available on a handle with a deflation";
    if (h->precond == DPCG_PRECOND_CALLBACK)
        return "dpcg_solve: the callback preconditioner is not available on a handle with a deflation (updates are enqueued ahead of the test)";
    if (h->ns) return "dpcg_solve: the handle has both a null space and a deflation";
    return nullptr;
}

// dpcg_update_values: the span stays; A W and the A-orthonormalisation are redone for the new values
int deflation_values_changed(dpcg_system *h, hipStream_t s) {
    if (!h->df) return DPCG_OK;
    const int st = a_orthonormalise(h, h->df, "dpcg_update_values (the deflation has been dropped)", s);
    if (st < 0) free_deflation(h);
    return st;
}

extern "C" int dpcg_set_deflation(dpcg_handle_t h, int k, const double *W, int memspace, dpcg_stream_t stream) {
    if (!h) return invalid("dpcg_set_deflation: NULL handle");
    if (k < 0 || k > kDfMaxK) return invalid("dpcg_set_deflation: k must lie in 0 .. 8 (0 clears)");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);            // (the old vectors may be in use on another stream)
    if (k == 0) {
        free_deflation(h);
        return DPCG_OK;
    }
    if (!W) return invalid("dpcg_set_deflation: W is NULL");
    if (memspace != DPCG_HOST && memspace != DPCG_DEVICE) return invalid("dpcg_set_deflation: bad memspace");
    if (h->ns) return invalid("dpcg_set_deflation: the handle has a null space attached (dpcg_set_nullspace): one or the other");
    const int64_t n = h->A.n;
    if (k > n) return invalid("dpcg_set_deflation: more columns than rows");
    Deflation *df = new Deflation();
    df->k = k;
    df->kp = k <= 2 ? k : (k <= 4 ? 4 : 8);
    df->ld = (n + kDfSpan - 1) / kDfSpan * kDfSpan;
    auto fail = [&](int st) {
        release(df);
        return st;
    };
    std::vector<double> Q((size_t)n * k);
    if (memspace == DPCG_HOST) {
        memcpy(Q.data(), W, Q.size() * sizeof(double));
    } else {
        hipError_t e = hipMemcpyAsync(Q.data(), W, Q.size() * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_deflation: reading W", __FILE__, __LINE__));
    }
    for (size_t i = 0; i < Q.size(); ++i)
        if (!std::isfinite(Q[i])) return fail(invalid("dpcg_set_deflation: W holds a non-finite entry"));
    // to the handle's numbering (row i of the handle = row perm[i] of the caller), columns ld apart, the padding rows and columns zero
    int st = DPCG_OK;
    std::vector<int32_t> perm;
    if ((st = read_perm(h, perm, s)) < 0) return fail(st);
    std::vector<double> Wp((size_t)df->ld * df->kp, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < n; ++i) Wp[(size_t)j * df->ld + i] = Q[(size_t)j * n + (perm.empty() ? i : perm[(size_t)i])];
    const int64_t total = df->ld * df->kp;
    if ((st = dev_alloc(&df->W, total)) < 0 || (st = dev_alloc(&df->AW, total)) < 0) return fail(st);
    if ((st = dev_alloc(&df->part, (int64_t)kDfSlots * kMaxGrid)) < 0) return fail(st);
    if ((st = dev_alloc(&df->gs_part, (int64_t)k * (df->ld / 128))) < 0) return fail(st);
    if ((st = dev_alloc(&df->coef, kDfCoefCount)) < 0) return fail(st);
    hipError_t e = hipMemcpyAsync(df->W, Wp.data(), Wp.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(df->AW, 0, (size_t)total * sizeof(double), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);       // (Wp goes out of scope)
    if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_deflation: uploading W", __FILE__, __LINE__));
    if ((st = a_orthonormalise(h, df, "dpcg_set_deflation", s)) < 0) return fail(st);
    free_deflation(h);
    h->df = df;
    return DPCG_OK;
}

extern "C" int dpcg_get_deflation(dpcg_handle_t h, int *k, double *W_host, double *AW_host) {
    if (!h || !k) return invalid("dpcg_get_deflation: NULL argument");
    const Deflation *df = h->df;
    *k = df ? df->k : 0;
    if (!df || (!W_host && !AW_host)) return DPCG_OK;
    DPCG_HIP(device_wide_wait());                         // (no stream argument: whatever stream the attach ran on)
    const int64_t n = h->A.n;
    std::vector<int32_t> perm;
    DPCG_TRY(read_perm(h, perm, nullptr));
    std::vector<double> tmp((size_t)n * df->k);
    const size_t width = (size_t)n * sizeof(double), pitch = (size_t)df->ld * sizeof(double);
    for (int which = 0; which < 2; ++which) {
        double *out = which == 0 ? W_host : AW_host;
        if (!out) continue;
        DPCG_HIP(hipMemcpy2D(tmp.data(), width, which == 0 ? df->W : df->AW, pitch, width, (size_t)df->k, hipMemcpyDeviceToHost));
        for (int j = 0; j < df->k; ++j)
            for (int64_t i = 0; i < n; ++i) out[(size_t)j * n + (perm.empty() ? i : perm[(size_t)i])] = tmp[(size_t)j * n + i];
    }
    return DPCG_OK;
}

// The solve of a handle with a deflation, whatever its size: plain launches enqueued ahead of the progress word that K3d posts (the
// kernels of an update enqueued beyond the stop return at once, as in the plain driver).
int solve_deflated_one(dpcg_system *h, SolveCall c) {
    Deflation *df = h->df;
    const int64_t n = h->A.n;
    hipStream_t s = c.s;
    const int G = h->vec_grid;
    HandleExtras &ex = extras()[h];
    DPCG_TRY(ensure_work(h, c.max_iter, false, false));
    *ex.prog_host = 0;
    const double *b = c.b;
    if (h->perm) {                         // b and x0 arrive in the caller's numbering
        if (!h->pb) DPCG_TRY(dev_alloc(&h->pb, n));
        launch_gather_f64(n, h->perm, b, h->pb, s);
        b = h->pb;
    }
    if (c.x0) {
        if (h->perm) launch_gather_f64(n, h->perm, c.x0, h->x, s);
        else DPCG_HIP(hipMemcpyAsync(h->x, c.x0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        launch_spmv(h->A, h->planA, h->x, h->q, nullptr, nullptr, s);
        launch_residual(n, b, h->q, h->r, G, s);                                       // r = b - A x0
    } else {
        DPCG_HIP(hipMemsetAsync(h->x, 0, (size_t)n * sizeof(double), s));
        DPCG_HIP(hipMemcpyAsync(h->r, b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
#define DPCG_DF_L(KV)                                                                                                      \
    hipLaunchKernelGGL((k_df_wt_dots<KV>), dim3(G), dim3(kBlock), 0, s, n, h->r, df->W, df->ld, df->part);                   \
    hipLaunchKernelGGL((k_df_correct<KV>), dim3(G), dim3(kBlock), 0, s, n, h->x, h->r, df->W, df->AW, df->ld, df->part, G)
    DPCG_DF_SHAPES(df, DPCG_DF_L);                                                     // c = W^T r;  x += W c;  r -= AW c
#undef DPCG_DF_L
    const double *z = h->precond == DPCG_PRECOND_NONE ? h->r : h->z;
    if (h->precond != DPCG_PRECOND_NONE) DPCG_TRY(apply_precond(h, h->r, h->z, s));
    const int init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    launch_df_dots(h, nullptr, h->r, z, b, true, init_check_r, s);
#define DPCG_DF_L(KV)                                                                                                       \
    hipLaunchKernelGGL((k_df_init<KV>), dim3(G), dim3(kBlock), 0, s, n, h->scal, df->part, G, z, h->p, df->W, df->ld, c.rtol_sq, \
                       c.atol_sq, h->hist, h->hist_cap, ex.prog_dev)
    DPCG_DF_SHAPES(df, DPCG_DF_L);
#undef DPCG_DF_L
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
            DPCG_TRY(enqueue_df_update(h, s));
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
            set_error("PCG driver (deflation): enqueued updates finished without reporting progress");
            return DPCG_ERR_STATE;
        }
    }
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
