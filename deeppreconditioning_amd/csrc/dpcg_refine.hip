// Mixed-precision PCG (dpcg_solve_refined, include/dpcg.h): an inner PCG whose matrix values and vectors are all STORED in fp32, inside an
// fp64 loop that recomputes the true residual and corrects x (iterative refinement).  Not in the reference.  Compiled with
// -ffp-contract=off like dpcg_pcg.hip.  Storage is fp32 and arithmetic is fp64, the convention of the fp32 AMG cycle: every product and sum
// is formed in fp64 and a value is rounded to fp32 exactly where it is stored to an fp32 vector; the dots run over the stored values.
//
// Launches of an inner update, M = I / Jacobi -- the three of a plain solve, over 4-byte entries:
//   K1  k_rf_spmv:       q = fl32(A32 p) by CSR rows with the planner's lanes-per-row rule, per-workgroup partials of <p,q>
//   K2  k_rf_update_r:   alpha;  r = fl32(r - alpha q);  z = fl32(dinv32 r) on the fly;  per-workgroup partials of <r,r> and <r,z>
//   K3  k_rf_update_dp:  those sums re-reduced in one fixed order by every workgroup;  rho', beta;  workgroup 0 records the history and
//                        runs the test;  d = fl32(d + alpha p);  p = fl32(z + beta p), z formed again from the stored r
// K2 and K3 move four floats a lane in 16-byte accesses, the next group requested before the current one is consumed.  The control
// words (done, done_seen, k, the progress word) are the plain solve's (Scalars, record_and_test), the host keeps updates enqueued ahead
// of the progress word (run_launch_ahead), every kernel returns at once when `done` is set.  No float atomics: wave tree, four wave
// sums in LDS, the partials in a fixed order (block_sum_n, reduce_slots, store_slots of dpcg_projected.h).
// An outer step: the handle's fp64 SpMV;  k_rf_residual (r = b - A x, partials of <r,r> and <b,b>);  k_rf_sums brings the two sums to
// the host, which runs the outer tests and forms sigma and the inner target;  k_rf_start (r32 = fl32(r / sigma), d = 0, p = z, the
// partials of the inner <r,r> and <r,z>: sigma needs the whole of <r,r>, so forming r and scaling it are two passes);  k_rf_init (the
// control words and the first test);  the inner updates;  k_rf_add_x (x += sigma d).
// The SpMV is a row kernel of its own and not dpcg_spmv.hip's fp32 form (config C5): that one stores q in fp64 and sums <p,q> against an
// fp64 p; here q is rounded where it is stored and <p,q> runs over the stored q.  The fp32 copies are made by k_rf_to_f32, which also
// reports the first entry that is not finite after rounding; the AMG's own conversion kernel is local to dpcg_amg.hip and stays there.
#include <chrono>
#include <cmath>
#include <limits>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_projected.h"

namespace dpcg {

// partial slots, kMaxGrid doubles each (the inner solve: <r,r>, <r,z>; the outer residual: <r,r>, <b,b>)
constexpr int kRfSlotRR = 0, kRfSlotRZ = 1, kRfSlotBB = 1, kRfSlots = 2;
constexpr unsigned long long kRfNoBad = ~0ull;

struct Refine {
    float *val32 = nullptr;         // fl32 of A's values, the handle's numbering
    float *dinv32 = nullptr;        // fl32 of the reciprocal diagonal (Jacobi only)
    float *r = nullptr, *d = nullptr, *p = nullptr, *q = nullptr;     // n floats each
    double *part = nullptr;         // kRfSlots x kMaxGrid
    double *sums = nullptr;         // the two sums of an outer residual, for the host
    unsigned long long *bad = nullptr;   // first entry that is not finite in fp32 (kRfNoBad: none)
    int tpr = 2, spmv_grid = 1;     // lanes per row and workgroups of K1
};

namespace {

typedef float Float2 __attribute__((ext_vector_type(2)));
typedef int Int2 __attribute__((ext_vector_type(2)));

// out = fl32(in);  *bad = the smallest index whose rounded value is not finite
__global__ __launch_bounds__(kBlock) void k_rf_to_f32(int64_t n, const double *__restrict__ in, float *__restrict__ out,
                                                      unsigned long long *__restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float f = (float)in[i];
        out[i] = f;
        if (!(f - f == 0.0f)) atomicMin(bad, (unsigned long long)i);
    }
}

// K1.  TPR lanes share a row, each takes aligned pairs of consecutive non-zeros (8-byte value and column loads) where both lie in the
// row, a shuffle tree combines the lanes.  The head of an update: returns at once when the solve is done, rotates rz_next -> rz.
template <int TPR>
__global__ __launch_bounds__(kBlock) void k_rf_spmv(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const float *__restrict__ val, const float *__restrict__ p, float *__restrict__ q,
                                                    double *__restrict__ part_pq, IterCtlDev ctl) {
    __shared__ double sh[4];
    if (!iteration_head(ctl)) return;
    constexpr int RPB = kBlock / TPR;
    const int t = threadIdx.x;
    const int lane = t % TPR;
    const int v = virtual_block();
    const int ngroups = (int)((n + RPB - 1) / RPB);
    int g_lo, g_hi;
    split_range(ngroups, v, g_lo, g_hi);
    double acc = 0.0;
    for (int g = g_lo; g < g_hi; ++g) {
        const int64_t row = (int64_t)g * RPB + t / TPR;
        double s = 0.0;
        if (row < n) {
            const int rs = rowptr[row], re = rowptr[row + 1];
            for (int k = (rs & ~1) + 2 * lane; k < re; k += 2 * TPR) {
                if (k + 1 < re) {
                    const Float2 av = *reinterpret_cast<const Float2 *>(val + k);
                    const Int2 cv = *reinterpret_cast<const Int2 *>(col + k);
                    if (k >= rs) s += (double)av.x * (double)p[cv.x];
                    s += (double)av.y * (double)p[cv.y];
                } else if (k >= rs) {                                   // the row's last entry alone (nothing is read beyond it)
                    s += (double)val[k] * (double)p[col[k]];
                }
            }
        }
#pragma unroll
        for (int off = TPR / 2; off > 0; off >>= 1) s += __shfl_down(s, off, TPR);
        if (lane == 0 && row < n) {
            const float qs = (float)s;
            q[row] = qs;
            acc += (double)p[row] * (double)qs;
        }
    }
    const double tot = block_sum(acc, sh);
    if (t == 0) part_pq[blockIdx.x] = tot;
}

// K2.  JAC: z = fl32(dinv32 r), not stored (K3 forms the same product again); else z = r.
template <bool JAC>
__global__ __launch_bounds__(kBlock) void k_rf_update_r(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part_pq,
                                                        int n_part_pq, const float *__restrict__ q, float *__restrict__ r,
                                                        const float *__restrict__ dinv, double *__restrict__ part) {
    __shared__ double sh[4 * kRfSlots];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const float4 *__restrict__ q4 = reinterpret_cast<const float4 *>(q);
    const float4 *__restrict__ d4 = reinterpret_cast<const float4 *>(dinv);
    float4 *__restrict__ r4 = reinterpret_cast<float4 *>(r);
    float4 qa = make_float4(0, 0, 0, 0), ra = qa, da = qa;
    bool have = i < n4;
    if (have) {
        qa = q4[i];
        ra = r4[i];
        if (JAC) da = d4[i];
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
    double acc[kRfSlots] = {0.0, 0.0};
    auto one = [&](float rc, float qc, float dc) -> float {
        const float rn = (float)((double)rc - alpha * (double)qc);
        const double rd = (double)rn;
        acc[kRfSlotRR] += rd * rd;
        const double zd = JAC ? (double)(float)((double)dc * rd) : rd;
        acc[kRfSlotRZ] += rd * zd;
        return rn;
    };
    while (have) {
        const int64_t cur = i;
        const float4 qc = qa, rc = ra, dc = da;
        i += stride;
        have = i < n4;
        if (have) {
            qa = q4[i];
            ra = r4[i];
            if (JAC) da = d4[i];
        }
        float4 rn;
        rn.x = one(rc.x, qc.x, dc.x);
        rn.y = one(rc.y, qc.y, dc.y);
        rn.z = one(rc.z, qc.z, dc.z);
        rn.w = one(rc.w, qc.w, dc.w);
        r4[cur] = rn;
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {            // the tail: n % 4 entries, one lane each
        const int64_t e = 4 * n4 + threadIdx.x;
        r[e] = one(r[e], q[e], JAC ? dinv[e] : 0.0f);
    }
    block_sum_n<kRfSlots>(acc, sh);
    if (threadIdx.x == 0) store_slots<kRfSlots>(part, 0, acc);
}

// K3
template <bool JAC>
__global__ __launch_bounds__(kBlock) void k_rf_update_dp(int64_t n, Scalars *__restrict__ sc, const double *__restrict__ part, int G,
                                                         const float *__restrict__ r, const float *__restrict__ dinv,
                                                         float *__restrict__ p, float *__restrict__ d, double *__restrict__ hist,
                                                         int hist_cap) {
    __shared__ double sh[4 * kRfSlots];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(r);
    const float4 *__restrict__ v4 = reinterpret_cast<const float4 *>(dinv);
    float4 *__restrict__ p4 = reinterpret_cast<float4 *>(p);
    float4 *__restrict__ d4 = reinterpret_cast<float4 *>(d);
    float4 ra = make_float4(0, 0, 0, 0), pa = ra, xa = ra, va = ra;
    bool have = i < n4;
    if (have) {
        ra = r4[i];
        pa = p4[i];
        xa = d4[i];
        if (JAC) va = v4[i];
    }
    // `done_seen`, not `done` (see k_update_xp): workgroup 0 of THIS launch sets `done`
    const int done_seen = sc->done_seen;
    double rz_old = sc->rz, alpha = sc->alpha;
    pin_scalar(rz_old);
    pin_scalar(alpha);
    if (done_seen) return;
    double v[kRfSlots];
    reduce_slots<kRfSlots>(part, 0, G, v, sh);
    const double rz_new = v[kRfSlotRZ];
    const double beta = rz_new / rz_old;
    if (blockIdx.x == 0 && threadIdx.x == 0) record_and_test(sc, v[kRfSlotRR], rz_new, hist, hist_cap, sc->k + 1);
    auto one = [&](float rc, float vc, float pc, float xc, float &pn) -> float {
        const double zd = JAC ? (double)(float)((double)vc * (double)rc) : (double)rc;
        pn = (float)(zd + beta * (double)pc);
        return (float)((double)xc + alpha * (double)pc);
    };
    while (have) {
        const int64_t cur = i;
        const float4 rc = ra, pc = pa, xc = xa, vc = va;
        i += stride;
        have = i < n4;
        if (have) {
            ra = r4[i];
            pa = p4[i];
            xa = d4[i];
            if (JAC) va = v4[i];
        }
        float4 xn, pn;
        xn.x = one(rc.x, vc.x, pc.x, xc.x, pn.x);
        xn.y = one(rc.y, vc.y, pc.y, xc.y, pn.y);
        xn.z = one(rc.z, vc.z, pc.z, xc.z, pn.z);
        xn.w = one(rc.w, vc.w, pc.w, xc.w, pn.w);
        d4[cur] = xn;
        p4[cur] = pn;
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
        const int64_t e = 4 * n4 + threadIdx.x;
        float pn;
        d[e] = one(r[e], JAC ? dinv[e] : 0.0f, p[e], d[e], pn);
        p[e] = pn;
    }
}

// The outer residual: r = b - ax (ax null: r = b) with the partials of <r,r> and <b,b>
__global__ __launch_bounds__(kBlock) void k_rf_residual(int64_t n, const double *__restrict__ b, const double *__restrict__ ax,
                                                        double *__restrict__ r, double *__restrict__ part) {
    __shared__ double sh[4 * kRfSlots];
    double acc[kRfSlots] = {0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double bi = b[i];
        const double ri = ax ? bi - ax[i] : bi;
        r[i] = ri;
        acc[kRfSlotRR] += ri * ri;
        acc[kRfSlotBB] += bi * bi;
    }
    block_sum_n<kRfSlots>(acc, sh);
    if (threadIdx.x == 0) store_slots<kRfSlots>(part, 0, acc);
}

// one workgroup: the two sums a kernel left in the slots, for the host
__global__ __launch_bounds__(kBlock) void k_rf_sums(const double *__restrict__ part, int G, double *__restrict__ out) {
    __shared__ double sh[4 * kRfSlots];
    double v[kRfSlots];
    reduce_slots<kRfSlots>(part, 0, G, v, sh);
    if (threadIdx.x == 0) {
        out[0] = v[0];
        out[1] = v[1];
    }
}

// The start of an inner solve: r32 = fl32(r / sigma), d = 0, p = z = fl32(dinv32 r32), the partials of <r32,r32> and <r32,z>.
// Four entries a lane: two 16-byte loads of r, 16-byte stores.
template <bool JAC>
__global__ __launch_bounds__(kBlock) void k_rf_start(int64_t n, const double *__restrict__ r, double sigma, const float *__restrict__ dinv,
                                                     float *__restrict__ r32, float *__restrict__ p, float *__restrict__ d,
                                                     double *__restrict__ part) {
    __shared__ double sh[4 * kRfSlots];
    double acc[kRfSlots] = {0.0, 0.0};
    auto one = [&](double ri, float dc, float &pn) -> float {
        const float rs = (float)(ri / sigma);
        const double rd = (double)rs;
        const float z = JAC ? (float)((double)dc * rd) : rs;
        acc[kRfSlotRR] += rd * rd;
        acc[kRfSlotRZ] += rd * (double)z;
        pn = z;
        return rs;
    };
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const double2 *__restrict__ rr2 = reinterpret_cast<const double2 *>(r);
    const float4 *__restrict__ v4 = reinterpret_cast<const float4 *>(dinv);
    const float4 zero = make_float4(0, 0, 0, 0);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        const double2 a = rr2[2 * i], c = rr2[2 * i + 1];
        const float4 vc = JAC ? v4[i] : zero;
        float4 rn, pn;
        rn.x = one(a.x, vc.x, pn.x);
        rn.y = one(a.y, vc.y, pn.y);
        rn.z = one(c.x, vc.z, pn.z);
        rn.w = one(c.y, vc.w, pn.w);
        reinterpret_cast<float4 *>(r32)[i] = rn;
        reinterpret_cast<float4 *>(p)[i] = pn;
        reinterpret_cast<float4 *>(d)[i] = zero;
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
        const int64_t e = 4 * n4 + threadIdx.x;
        float pn;
        r32[e] = one(r[e], JAC ? dinv[e] : 0.0f, pn);
        p[e] = pn;
        d[e] = 0.0f;
    }
    block_sum_n<kRfSlots>(acc, sh);
    if (threadIdx.x == 0) store_slots<kRfSlots>(part, 0, acc);
}

// one workgroup: the control words of an inner solve and its first test, on <r32,r32> / <r32,r32> (DPCG_INIT_CHECK_R)
__global__ __launch_bounds__(kBlock) void k_rf_init(Scalars *sc, const double *__restrict__ part, int G, double target, double *hist,
                                                    int hist_cap, unsigned long long *progress) {
    __shared__ double sh[4 * kRfSlots];
    double v[kRfSlots];
    reduce_slots<kRfSlots>(part, 0, G, v, sh);
    if (threadIdx.x == 0) {
        sc->bb = v[kRfSlotRR];
        sc->rz = v[kRfSlotRZ];
        sc->alpha = 0.0;
        sc->rtol_sq = target;
        sc->atol_sq = 0.0;
        sc->done = 0;
        sc->status = DPCG_MAX_ITER;
        sc->done_seen = 0;
        sc->progress = progress;
        record_and_test(sc, v[kRfSlotRR], v[kRfSlotRZ], hist, hist_cap, 0);
    }
}

// x += sigma d
__global__ __launch_bounds__(kBlock) void k_rf_add_x(int64_t n, double sigma, const float *__restrict__ d, double *__restrict__ x) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        const float4 dc = reinterpret_cast<const float4 *>(d)[i];
        double2 a = x2[2 * i], c = x2[2 * i + 1];
        a.x = a.x + sigma * (double)dc.x;
        a.y = a.y + sigma * (double)dc.y;
        c.x = c.x + sigma * (double)dc.z;
        c.y = c.y + sigma * (double)dc.w;
        x2[2 * i] = a;
        x2[2 * i + 1] = c;
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) {
        const int64_t e = 4 * n4 + threadIdx.x;
        x[e] = x[e] + sigma * (double)d[e];
    }
}

void release(Refine *rf) {
    if (!rf) return;
    dev_free(rf->val32);
    dev_free(rf->dinv32);
    dev_free(rf->r);
    dev_free(rf->d);
    dev_free(rf->p);
    dev_free(rf->q);
    dev_free(rf->part);
    dev_free(rf->sums);
    dev_free(rf->bad);
    delete rf;
}

// out = fl32(in) on the device; a rounded entry that is not finite is refused by name
int to_f32_checked(Refine *rf, int64_t count, const double *in, float *out, const char *what, hipStream_t s) {
    unsigned long long bad = kRfNoBad;
    DPCG_HIP(hipMemcpyAsync(rf->bad, &bad, sizeof(bad), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rf_to_f32, dim3(grid_for(count)), dim3(kBlock), 0, s, count, in, out, rf->bad);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipMemcpyAsync(&bad, rf->bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    if (bad != kRfNoBad) {
        double v = 0.0;
        DPCG_HIP(hipMemcpy(&v, in + bad, sizeof(double), hipMemcpyDeviceToHost));
        char buf[256];
        snprintf(buf, sizeof(buf), "dpcg_solve_refined: %s %llu (%.17g, the handle's numbering) is not finite after rounding to fp32", what, bad, v);
        set_error(buf);
        return DPCG_ERR_INVALID;
    }
    return DPCG_OK;
}

// The fp32 copies and work vectors, made by the first call.  Built into a local and attached only when all of it exists: a refusal
// leaves the handle as it was.
int ensure_refine(dpcg_system *h, hipStream_t s) {
    if (h->rf) return DPCG_OK;
    const int64_t n = h->A.n;
    Refine *rf = new Refine();
    auto fail = [&](int st) {
        release(rf);
        return st;
    };
    int st = DPCG_OK;
    if ((st = dev_alloc(&rf->bad, 1)) < 0 || (st = dev_alloc(&rf->val32, h->A.nnz)) < 0) return fail(st);
    if ((st = to_f32_checked(rf, h->A.nnz, h->A.val, rf->val32, "matrix value", s)) < 0) return fail(st);
    if (h->precond == DPCG_PRECOND_JACOBI) {
        if ((st = dev_alloc(&rf->dinv32, n)) < 0) return fail(st);
        if ((st = to_f32_checked(rf, n, h->dinv, rf->dinv32, "reciprocal diagonal entry", s)) < 0) return fail(st);
    }
    if ((st = dev_alloc(&rf->r, n)) < 0 || (st = dev_alloc(&rf->d, n)) < 0 || (st = dev_alloc(&rf->p, n)) < 0 ||
        (st = dev_alloc(&rf->q, n)) < 0)
        return fail(st);
    if ((st = dev_alloc(&rf->part, (int64_t)kRfSlots * kMaxGrid)) < 0 || (st = dev_alloc(&rf->sums, kRfSlots)) < 0) return fail(st);
    // lanes per row: the planner's rule (make_plan), a lane takes two non-zeros per trip
    const double mean = n > 0 ? (double)h->A.nnz / (double)n : 1.0;
    int tpr = 2;
    while (tpr < 64 && 2 * tpr < mean) tpr *= 2;
    rf->tpr = tpr;
    const int64_t ngroups = (n + (kBlock / tpr) - 1) / (kBlock / tpr);
    int g = ngroups < kMaxSpmvGrid ? (int)ngroups : kMaxSpmvGrid;
    if (g > 8) g -= g % 8;
    rf->spmv_grid = g < 1 ? 1 : g;
    h->rf = rf;
    return DPCG_OK;
}

void launch_rf_spmv(const dpcg_system *h, hipStream_t s) {
    const Refine *rf = h->rf;
    const IterCtlDev ctl{h->scal};
#define DPCG_RF_SPMV_CASE(TPRV)                                                                                                       \
    case TPRV:                                                                                                                        \
        hipLaunchKernelGGL((k_rf_spmv<TPRV>), dim3(rf->spmv_grid), dim3(kBlock), 0, s, h->A.n, h->A.rowptr, h->A.col, rf->val32, rf->p, \
                           rf->q, h->part_pq, ctl);                                                                                   \
        break
    switch (rf->tpr) {
        DPCG_RF_SPMV_CASE(2);
        DPCG_RF_SPMV_CASE(4);
        DPCG_RF_SPMV_CASE(8);
        DPCG_RF_SPMV_CASE(16);
        DPCG_RF_SPMV_CASE(32);
        default:
            DPCG_RF_SPMV_CASE(64);
    }
#undef DPCG_RF_SPMV_CASE
}

// one inner update as launches on s
int enqueue_refine_update(dpcg_system *h, hipStream_t s) {
    const Refine *rf = h->rf;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    launch_rf_spmv(h, s);                                                                                                  // K1
    if (rf->dinv32) {
        hipLaunchKernelGGL((k_rf_update_r<true>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, rf->spmv_grid, rf->q, rf->r,
                           rf->dinv32, rf->part);                                                                          // K2
        hipLaunchKernelGGL((k_rf_update_dp<true>), dim3(G), dim3(kBlock), 0, s, n, h->scal, rf->part, G, rf->r, rf->dinv32, rf->p, rf->d,
                           h->hist, h->hist_cap);                                                                          // K3
    } else {
        hipLaunchKernelGGL((k_rf_update_r<false>), dim3(G), dim3(kBlock), 0, s, n, h->scal, h->part_pq, rf->spmv_grid, rf->q, rf->r,
                           (const float *)nullptr, rf->part);
        hipLaunchKernelGGL((k_rf_update_dp<false>), dim3(G), dim3(kBlock), 0, s, n, h->scal, rf->part, G, rf->r, (const float *)nullptr,
                           rf->p, rf->d, h->hist, h->hist_cap);
    }
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

void free_refine(dpcg_system *h) {
    release(h->rf);
    h->rf = nullptr;
}

extern "C" int dpcg_solve_refined(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq, double atol_sq,
                                  int max_iter, double inner_rtol_sq, int max_outer, int flags, dpcg_stream_t stream, int *iters,
                                  int *outer, double *final_res, double *seconds, double *res_history, double *outer_history) {
    if (!h || !b) return invalid("dpcg_solve_refined: NULL handle or b");
    if (max_iter < 0) return invalid("dpcg_solve_refined: max_iter < 0");
    if (!(inner_rtol_sq > 0.0)) return invalid("dpcg_solve_refined: inner_rtol_sq must be > 0");
    if (max_outer < 1) return invalid("dpcg_solve_refined: max_outer < 1");
    if (flags & ~DPCG_NO_GRAPH) return invalid("dpcg_solve_refined: flags takes 0 or DPCG_NO_GRAPH only");
    if (h->precond != DPCG_PRECOND_NONE && h->precond != DPCG_PRECOND_JACOBI)
        return invalid("dpcg_solve_refined: the inner solve takes no preconditioner or Jacobi only");
    if (h->ns) return invalid("dpcg_solve_refined: the handle has a null space attached");
    if (h->df) return invalid("dpcg_solve_refined: the handle has a deflation attached");
    if (h->precond == DPCG_PRECOND_JACOBI && !h->dinv) return DPCG_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    DPCG_TRY(ensure_refine(h, s));
    Refine *rf = h->rf;
    const bool jac = rf->dinv32 != nullptr;
    DPCG_TRY(stage_vectors(h, b, x0, max_iter, false, false, s, &b));       // (the residual is formed below, with its sums)
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();
    volatile unsigned long long *prog = extras()[h].prog_host;
    std::vector<double> inner_hist;
    int total = 0, s_out = 0, status = DPCG_MAX_ITER, n_hist = 0;
    double rr_prev = 0.0, res = 0.0;
    for (;; ++s_out) {
        if (s_out > 0 || x0) launch_spmv(h->A, h->planA, h->x, h->q, nullptr, nullptr, s);
        hipLaunchKernelGGL(k_rf_residual, dim3(G), dim3(kBlock), 0, s, n, b, (s_out > 0 || x0) ? h->q : (const double *)nullptr, h->r,
                           rf->part);
        hipLaunchKernelGGL(k_rf_sums, dim3(1), dim3(kBlock), 0, s, rf->part, G, rf->sums);
        DPCG_CHECK_LAUNCH();
        double sums[kRfSlots];
        DPCG_HIP(hipMemcpyAsync(sums, rf->sums, sizeof(sums), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        const double rr = sums[kRfSlotRR], bb = sums[kRfSlotBB];
        res = rr / bb;
        if (outer_history) outer_history[s_out] = res;
        if (s_out == 0 && res_history) res_history[n_hist++] = res;
        if (res < rtol_sq || rr < atol_sq) {
            status = DPCG_OK;
            break;
        }
        if (total == max_iter || s_out == max_outer) break;
        if (!std::isfinite(rr) || !(res == res)) {
            status = DPCG_BREAKDOWN;
            break;
        }
        if (s_out >= 1 && rr >= 0.25 * rr_prev) {
            set_error("dpcg_solve_refined: stagnated (an outer step reduced <r,r> by less than a factor 4)");
            break;
        }
        rr_prev = rr;
        const double sigma = std::sqrt(rr);
        const double target = std::max(inner_rtol_sq, 0.25 * rtol_sq * bb / rr);
        const int cap = max_iter - total;
        *prog = 0;
        if (jac) hipLaunchKernelGGL((k_rf_start<true>), dim3(G), dim3(kBlock), 0, s, n, h->r, sigma, rf->dinv32, rf->r, rf->p, rf->d, rf->part);
        else hipLaunchKernelGGL((k_rf_start<false>), dim3(G), dim3(kBlock), 0, s, n, h->r, sigma, (const float *)nullptr, rf->r, rf->p, rf->d, rf->part);
        hipLaunchKernelGGL(k_rf_init, dim3(1), dim3(kBlock), 0, s, h->scal, rf->part, G, target, h->hist, h->hist_cap, extras()[h].prog_dev);
        DPCG_CHECK_LAUNCH();
        DPCG_TRY(run_launch_ahead(h, cap, s, std::chrono::steady_clock::now(), " (refined)", [&] { return enqueue_refine_update(h, s); }));
        launch_final_check(h->scal, s);
        hipLaunchKernelGGL(k_rf_add_x, dim3(G), dim3(kBlock), 0, s, n, sigma, rf->d, h->x);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipMemcpyAsync(h->scal_host, h->scal, sizeof(Scalars), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        const Scalars sc = *h->scal_host;
        if (res_history && sc.k > 0) {
            // entry t of the inner history is <r,r>_t / <r32,r32>: rescaled to <r,r>_t * rr / bb
            inner_hist.resize((size_t)sc.k);
            DPCG_HIP(hipMemcpy(inner_hist.data(), h->hist + 1, (size_t)sc.k * sizeof(double), hipMemcpyDeviceToHost));
            for (int t = 0; t < sc.k; ++t) res_history[n_hist++] = inner_hist[(size_t)t] * sc.bb * rr / bb;
        }
        total += sc.k;
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
    if (iters) *iters = total;
    if (outer) *outer = s_out;
    if (final_res) *final_res = res;
    if (x) DPCG_TRY(hand_over_x(h, x, s));
    DPCG_CHECK_LAUNCH();
    return status;
}
