// Right-preconditioned BiCGStab (dpcg_solve_bicgstab, include/dpcg.h; van der Vorst 1992) for systems whose values are not symmetric.
// Not in the reference.  Compiled with -ffp-contract=off like dpcg_pcg.hip.  A multi-launch driver of its own: no existing solve takes it.
//
//     r0 = b - A x0;  rhat = r0;  rho = alpha = omega = 1;  v = p = 0
//     update k:  rho' = <rhat,r>;  beta = (rho'/rho)(alpha/omega);  p = r + beta (p - omega v);  ph = M p;  v = A ph;  alpha = rho' / <rhat,v>
//                s = r - alpha v;  <s,s> meets the test: x += alpha ph, stop;  sh = M s;  t = A sh;  omega = <t,s>/<t,t>
//                x += alpha ph + omega sh;  r = s - omega t
// Launches of an update, M = I / Jacobi:
//   P   k_bi_pass_p:  <r,r> and <rhat,r> re-reduced by every workgroup in one fixed order;  workgroup 0 records the history and runs the test
//                     on r;  beta;  p = r + beta (p - omega v);  Jacobi: ph = dinv o p              reads r, p, v (dinv), writes p (ph)
//   A1  the handle's SpMV v = A ph, its epilogue leaves the partials of <rhat,v> (launch_spmv_xdot: every plan has it)
//   S   k_bi_pass_s:  alpha;  s = r - alpha v;  Jacobi: sh = dinv o s;  partials of <s,s>            reads r, v (dinv), writes s (sh)
//   A2  the handle's SpMV t = A sh, its epilogue leaves the partials of <s,t>
//   T   k_bi_tt:      partials of <t,t> (the SpMV's epilogue sums against one vector only)           reads t
//   X   k_bi_pass_x:  <s,s>, <s,t>, <t,t> re-reduced;  the half-step exit (x += alpha ph only);  omega;  x += alpha ph + omega sh;
//                     r = s - omega t;  partials of <rhat,r> and <r,r>                               reads x, ph, sh, s, t, rhat, writes x, r
// M = I: ph is p and sh is s (nothing stored twice).  Any other M: the handle's apply (apply_precond, in the loop) after P and after S.
// The passes move two doubles a lane in 16-byte accesses, the next pair requested before the current one is consumed; an odd n leaves one
// entry to one lane of workgroup 0.  The grid is grid_for(n) = ceil(n / 256) workgroups, 1024 at the most, so a lane takes a second pair
// -- the hand-over of the pipelined loops -- only from n > 2 x 256 x 1024 = 524 288 on (tests/test_bicgstab_edges_gpu.py runs 525 625
// rows, and small systems on 1 and 3 workgroups).  No float atomics: wave tree, four wave sums in LDS, the partials in a fixed order (block_sum_n,
// reduce_slots of dpcg_projected.h).
// Control.  The scalars rho, alpha, omega live in a device record (BiRec); the decisions -- the test on r, the half-step exit, the
// breakdowns -- are derived by EVERY workgroup from the same partials, so all of them agree without a hand-off; workgroup 0 writes them
// down.  No kernel reads a word that the same launch writes: P reads go_p (written by X and the start), S reads go_s (by P), X reads go_x
// (by S).  A pass that finds its word 0 clears the next one and returns, so the updates enqueued beyond the stop are no-ops -- but for
// their two SpMVs, which have no control word and run in full (their results are read by nobody).  The host keeps 3 .. 32 updates
// enqueued ahead, so a solve pays for up to 64 idle SpMVs after its stop and `seconds` includes them: a cost that counts for short
// solves of large systems.  Scalars::done, k, status, res and the progress word keep their
// meaning for the host pieces every launch-path driver shares (run_launch_ahead, deliver_solve, the in-loop skip of the applies).
#include <chrono>
#include <cmath>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_projected.h"

namespace dpcg {

// partial slots of the vector passes, kMaxGrid doubles each: <r,r>, <rhat,r> (pass X, the start), <s,s> (pass S; the start parks <b,b>
// there), <t,t> (k_bi_tt)
constexpr int kBiSlotRR = 0, kBiSlotRho = 1, kBiSlotSS = 2, kBiSlotTT = 3, kBiSlots = 4;

struct BiRec {
    double rho;        // <rhat,r> of the previous update (1 before the first), committed by pass S
    double rho_new;    // <rhat,r> of this update, written by pass P for pass S
    double alpha;      // written by pass S
    double omega;      // written by pass X
    int go_p, go_s, go_x;   // see the head of this file
};

struct BiCgStab {
    double *rhat = nullptr, *s = nullptr, *sh = nullptr, *t = nullptr;     // n doubles each (sh: null until a call has an M to apply)
    double *part = nullptr;                                                // kBiSlots x kMaxGrid
    double *part_rv = nullptr, *part_ts = nullptr;                         // the SpMV epilogues' partials, kMaxSpmvGrid each
    BiRec *rec = nullptr;
};

namespace {

__device__ __forceinline__ bool bi_finite(double v) { return v - v == 0.0; }

__device__ __forceinline__ void bi_post(Scalars *sc, int k, int done) {
    if (sc->progress)
        __hip_atomic_store(sc->progress, ((unsigned long long)k << 1) | (unsigned long long)done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one thread: the solve ends here with `status`, after `k` completed updates
__device__ __forceinline__ void bi_stop(Scalars *sc, int status, int k) {
    sc->status = status;
    sc->done = 1;
    bi_post(sc, k, 1);
}

// rhat = r, p = v = 0, the partials of <r,r> (twice: it is <rhat,r> too) and of <b,b> (parked in the <s,s> slot for k_bi_start)
__global__ __launch_bounds__(kBlock) void k_bi_init(int64_t n, const double *__restrict__ b, const double *__restrict__ r,
                                                    double *__restrict__ rhat, double *__restrict__ p, double *__restrict__ v,
                                                    double *__restrict__ part) {
    __shared__ double sh[4 * 2];
    double acc[2] = {0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ri = r[i], bi = b[i];
        rhat[i] = ri;
        p[i] = 0.0;
        v[i] = 0.0;
        acc[0] += ri * ri;
        acc[1] += bi * bi;
    }
    block_sum_n<2>(acc, sh);
    if (threadIdx.x == 0) {
        part[(int64_t)kBiSlotRR * kMaxGrid + blockIdx.x] = acc[0];
        part[(int64_t)kBiSlotRho * kMaxGrid + blockIdx.x] = acc[0];
        part[(int64_t)kBiSlotSS * kMaxGrid + blockIdx.x] = acc[1];
    }
}

// one workgroup: <b,b>, the control words and the record
__global__ __launch_bounds__(kBlock) void k_bi_start(Scalars *sc, BiRec *rec, const double *__restrict__ part, int G, double rtol_sq,
                                                     double atol_sq, unsigned long long *progress) {
    __shared__ double sh[4];
    double v[1];
    reduce_slots<1>(part, kBiSlotSS, G, v, sh);
    if (threadIdx.x == 0) {
        sc->rz = sc->rz_next = sc->alpha = sc->res = 0.0;
        sc->bb = v[0];
        sc->rtol_sq = rtol_sq;
        sc->atol_sq = atol_sq;
        sc->k = 0;
        sc->done = 0;
        sc->status = DPCG_MAX_ITER;
        sc->done_seen = 0;
        sc->progress = progress;
        rec->rho = rec->alpha = rec->omega = 1.0;
        rec->rho_new = 0.0;
        rec->go_p = 1;
        rec->go_s = rec->go_x = 0;
    }
}

// Pass P.  PRE: 0 = M = I (ph is p), 1 = Jacobi (ph = dinv o p), 2 = any other M (the apply follows).
template <int PRE>
__global__ __launch_bounds__(kBlock) void k_bi_pass_p(int64_t n, Scalars *__restrict__ sc, BiRec *__restrict__ rec,
                                                      const double *__restrict__ part, int G, const double *__restrict__ r,
                                                      double *__restrict__ p, const double *__restrict__ v,
                                                      const double *__restrict__ dinv, double *__restrict__ ph,
                                                      double *__restrict__ hist, int hist_cap) {
    __shared__ double sh[4 * 2];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ r2 = reinterpret_cast<const double2 *>(r);
    const double2 *__restrict__ v2 = reinterpret_cast<const double2 *>(v);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ p2 = reinterpret_cast<double2 *>(p);
    double2 *__restrict__ h2 = reinterpret_cast<double2 *>(ph);
    double2 ra = make_double2(0, 0), pa = ra, va = ra, da = ra;
    bool have = i < n2;
    if (have) {
        ra = r2[i];
        pa = p2[i];
        va = v2[i];
        if (PRE == 1) da = d2[i];
    }
    // the control word and the scalars travel with the first vector loads
    const int go = rec->go_p;
    double rho_old = rec->rho, alpha = rec->alpha, omega = rec->omega, bb = sc->bb, rtol_sq = sc->rtol_sq, atol_sq = sc->atol_sq;
    pin_scalar(rho_old);
    pin_scalar(alpha);
    pin_scalar(omega);
    pin_scalar(bb);
    pin_scalar(rtol_sq);
    pin_scalar(atol_sq);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!go) {
        if (first) rec->go_s = 0;
        return;
    }
    double sums[2];
    reduce_slots<2>(part, kBiSlotRR, G, sums, sh);
    const double rr = sums[0], rho_new = sums[1];
    const double res = rr / bb;
    const bool conv = (res < rtol_sq) || (rr < atol_sq);
    const bool broken = !(res == res) || rho_new == 0.0 || !bi_finite(rho_new);
    if (first) {
        const int k = sc->k;
        if (k < hist_cap) hist[k] = res;
        sc->res = res;
        if (conv) bi_stop(sc, DPCG_OK, k);
        else if (broken) bi_stop(sc, DPCG_BREAKDOWN, k);
        else rec->rho_new = rho_new;
        rec->go_s = (conv || broken) ? 0 : 1;
    }
    if (conv || broken) return;
    const double beta = (rho_new / rho_old) * (alpha / omega);
    while (have) {
        const int64_t cur = i;
        const double2 rc = ra, pc = pa, vc = va, dc = da;
        i += stride;
        have = i < n2;
        if (have) {
            ra = r2[i];
            pa = p2[i];
            va = v2[i];
            if (PRE == 1) da = d2[i];
        }
        double2 pn;
        pn.x = rc.x + beta * (pc.x - omega * vc.x);
        pn.y = rc.y + beta * (pc.y - omega * vc.y);
        p2[cur] = pn;
        if (PRE == 1) {
            double2 hn;
            hn.x = dc.x * pn.x;
            hn.y = dc.y * pn.y;
            h2[cur] = hn;
        }
    }
    if ((n & 1) && first) {                                             // odd tail element
        const int64_t e = n - 1;
        const double pn = r[e] + beta * (p[e] - omega * v[e]);
        p[e] = pn;
        if (PRE == 1) ph[e] = dinv[e] * pn;
    }
}

// Pass S.  PRE as in pass P (sh is s for M = I).
template <int PRE>
__global__ __launch_bounds__(kBlock) void k_bi_pass_s(int64_t n, Scalars *__restrict__ sc, BiRec *__restrict__ rec,
                                                      const double *__restrict__ part_rv, int n_part_rv, const double *__restrict__ r,
                                                      const double *__restrict__ v, const double *__restrict__ dinv,
                                                      double *__restrict__ s, double *__restrict__ shv, double *__restrict__ part) {
    __shared__ double sh[4];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double2 *__restrict__ r2 = reinterpret_cast<const double2 *>(r);
    const double2 *__restrict__ v2 = reinterpret_cast<const double2 *>(v);
    const double2 *__restrict__ d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *__restrict__ s2 = reinterpret_cast<double2 *>(s);
    double2 *__restrict__ h2 = reinterpret_cast<double2 *>(shv);
    double2 ra = make_double2(0, 0), va = ra, da = ra;
    bool have = i < n2;
    if (have) {
        ra = r2[i];
        va = v2[i];
        if (PRE == 1) da = d2[i];
    }
    // as k_update_r: the SpMV's partials and the control word travel with the first vector loads
    EarlyPartials<kSpmvPartSlots> ep;
    ep.request(part_rv, n_part_rv);
    const int go = rec->go_s;
    double rho = rec->rho_new;
    pin_scalar(rho);
    ep.land();
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!go) {
        if (first) rec->go_x = 0;
        return;
    }
    const double rv = ep.reduce(n_part_rv, sh);
    const bool broken = rv == 0.0 || !bi_finite(rv);
    const double alpha = rho / rv;
    if (first) {
        if (broken) {
            bi_stop(sc, DPCG_BREAKDOWN, sc->k);
        } else {
            rec->alpha = alpha;                                         // read by pass X and the next pass P (later kernels)
            rec->rho = rho;
        }
        rec->go_x = broken ? 0 : 1;
    }
    if (broken) return;
    double acc = 0.0;
    while (have) {
        const int64_t cur = i;
        const double2 rc = ra, vc = va, dc = da;
        i += stride;
        have = i < n2;
        if (have) {
            ra = r2[i];
            va = v2[i];
            if (PRE == 1) da = d2[i];
        }
        double2 sn;
        sn.x = rc.x - alpha * vc.x;
        sn.y = rc.y - alpha * vc.y;
        s2[cur] = sn;
        acc += sn.x * sn.x;
        acc += sn.y * sn.y;
        if (PRE == 1) {
            double2 hn;
            hn.x = dc.x * sn.x;
            hn.y = dc.y * sn.y;
            h2[cur] = hn;
        }
    }
    if ((n & 1) && first) {                                             // odd tail element
        const int64_t e = n - 1;
        const double sn = r[e] - alpha * v[e];
        s[e] = sn;
        acc += sn * sn;
        if (PRE == 1) shv[e] = dinv[e] * sn;
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(int64_t)kBiSlotSS * kMaxGrid + blockIdx.x] = tot;
}

// partials of <t,t>
__global__ __launch_bounds__(kBlock) void k_bi_tt(int64_t n, const BiRec *__restrict__ rec, const double *__restrict__ t,
                                                  double *__restrict__ part) {
    __shared__ double sh[4];
    if (!rec->go_x) return;
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const double2 *__restrict__ t2 = reinterpret_cast<const double2 *>(t);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) {
        const double2 tc = t2[i];
        acc += tc.x * tc.x;
        acc += tc.y * tc.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc += t[n - 1] * t[n - 1];
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(int64_t)kBiSlotTT * kMaxGrid + blockIdx.x] = tot;
}

// Pass X
__global__ __launch_bounds__(kBlock) void k_bi_pass_x(int64_t n, Scalars *__restrict__ sc, BiRec *__restrict__ rec,
                                                      const double *__restrict__ part_in, int G, const double *__restrict__ part_ts,
                                                      int n_part_ts, double *__restrict__ x, const double *__restrict__ ph,
                                                      const double *__restrict__ shv, const double *__restrict__ s,
                                                      const double *__restrict__ t, const double *__restrict__ rhat,
                                                      double *__restrict__ r, double *__restrict__ part_out, double *__restrict__ hist,
                                                      int hist_cap) {
    __shared__ double sh[4 * 2];
    const int64_t n2 = n >> 1;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double2 *__restrict__ x2 = reinterpret_cast<double2 *>(x);
    double2 *__restrict__ r2 = reinterpret_cast<double2 *>(r);
    const double2 *__restrict__ p2 = reinterpret_cast<const double2 *>(ph);
    const double2 *__restrict__ h2 = reinterpret_cast<const double2 *>(shv);
    const double2 *__restrict__ s2 = reinterpret_cast<const double2 *>(s);
    const double2 *__restrict__ t2 = reinterpret_cast<const double2 *>(t);
    const double2 *__restrict__ q2 = reinterpret_cast<const double2 *>(rhat);
    double2 xa = make_double2(0, 0), pa = xa, ha = xa, sa = xa, ta = xa, qa = xa;
    bool have = i < n2;
    if (have) {
        xa = x2[i];
        pa = p2[i];
        ha = h2[i];
        sa = s2[i];
        ta = t2[i];
        qa = q2[i];
    }
    EarlyPartials<kSpmvPartSlots> ep;
    ep.request(part_ts, n_part_ts);
    const int go = rec->go_x;
    double alpha = rec->alpha, bb = sc->bb, rtol_sq = sc->rtol_sq, atol_sq = sc->atol_sq;
    pin_scalar(alpha);
    pin_scalar(bb);
    pin_scalar(rtol_sq);
    pin_scalar(atol_sq);
    ep.land();
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!go) {
        if (first) rec->go_p = 0;
        return;
    }
    const double ts = ep.reduce(n_part_ts, sh);
    double sums[2];
    reduce_slots<2>(part_in, kBiSlotSS, G, sums, sh);
    const double ss = sums[0], tt = sums[1];
    const double res_s = ss / bb;
    const bool half = (res_s < rtol_sq) || (ss < atol_sq);
    if (half) {                                                         // the half-step exit: x += alpha ph, nothing else
        if (first) {
            const int k = sc->k + 1;
            if (k < hist_cap) hist[k] = res_s;
            sc->res = res_s;
            sc->k = k;
            rec->go_p = 0;
            bi_stop(sc, DPCG_OK, k);
        }
        while (have) {
            const int64_t cur = i;
            const double2 xc = xa, pc = pa;
            i += stride;
            have = i < n2;
            if (have) {
                xa = x2[i];
                pa = p2[i];
            }
            double2 xn;
            xn.x = xc.x + alpha * pc.x;
            xn.y = xc.y + alpha * pc.y;
            x2[cur] = xn;
        }
        if ((n & 1) && first) x[n - 1] = x[n - 1] + alpha * ph[n - 1];
        return;
    }
    const bool broken = tt == 0.0 || !bi_finite(tt) || !bi_finite(ts) || !bi_finite(ss);
    const double omega = ts / tt;
    if (first) {
        if (broken) {
            bi_stop(sc, DPCG_BREAKDOWN, sc->k);
        } else {
            const int k = sc->k + 1;
            rec->omega = omega;                                         // read by the next pass P (a later kernel)
            sc->k = k;
            bi_post(sc, k, 0);
        }
        rec->go_p = broken ? 0 : 1;
    }
    if (broken) return;
    double acc[2] = {0.0, 0.0};
    while (have) {
        const int64_t cur = i;
        const double2 xc = xa, pc = pa, hc = ha, sc2 = sa, tc = ta, qc = qa;
        i += stride;
        have = i < n2;
        if (have) {
            xa = x2[i];
            pa = p2[i];
            ha = h2[i];
            sa = s2[i];
            ta = t2[i];
            qa = q2[i];
        }
        double2 xn, rn;
        xn.x = (xc.x + alpha * pc.x) + omega * hc.x;
        xn.y = (xc.y + alpha * pc.y) + omega * hc.y;
        rn.x = sc2.x - omega * tc.x;
        rn.y = sc2.y - omega * tc.y;
        x2[cur] = xn;
        r2[cur] = rn;
        acc[0] += rn.x * rn.x;
        acc[0] += rn.y * rn.y;
        acc[1] += qc.x * rn.x;
        acc[1] += qc.y * rn.y;
    }
    if ((n & 1) && first) {                                             // odd tail element
        const int64_t e = n - 1;
        x[e] = (x[e] + alpha * ph[e]) + omega * shv[e];
        const double rn = s[e] - omega * t[e];
        r[e] = rn;
        acc[0] += rn * rn;
        acc[1] += rhat[e] * rn;
    }
    block_sum_n<2>(acc, sh);
    if (threadIdx.x == 0) store_slots<2>(part_out, kBiSlotRR, acc);
}

// one workgroup, after the last update the call allows: the test on the r that update left (max_iter = 0: on r0)
__global__ __launch_bounds__(kBlock) void k_bi_final(Scalars *sc, const BiRec *__restrict__ rec, const double *__restrict__ part, int G,
                                                     double *__restrict__ hist, int hist_cap) {
    __shared__ double sh[4];
    if (!rec->go_p) return;                                             // the solve has stopped: everything is written down
    double v[1];
    reduce_slots<1>(part, kBiSlotRR, G, v, sh);
    if (threadIdx.x == 0) {
        const double rr = v[0];
        const double res = rr / sc->bb;
        const int k = sc->k;
        if (k < hist_cap) hist[k] = res;
        sc->res = res;
        const bool conv = (res < sc->rtol_sq) || (rr < sc->atol_sq);
        bi_stop(sc, conv ? DPCG_OK : (!(res == res) ? DPCG_BREAKDOWN : DPCG_MAX_ITER), k);
    }
}

void release(BiCgStab *bi) {
    if (!bi) return;
    dev_free(bi->rhat);
    dev_free(bi->s);
    dev_free(bi->sh);
    dev_free(bi->t);
    dev_free(bi->part);
    dev_free(bi->part_rv);
    dev_free(bi->part_ts);
    dev_free(bi->rec);
    delete bi;
}

// The driver's own vectors and partial buffers, made by the first call and kept until the handle goes.  Attached only when all of it
// exists: a failure leaves the handle as it was.
int ensure_bicgstab(dpcg_system *h) {
    const int64_t n = h->A.n;
    if (h->bi) {                                                        // sh: made by the first call that has an M to apply
        if (precond_class(h) != 0 && !h->bi->sh) DPCG_TRY(dev_alloc(&h->bi->sh, n));
        return DPCG_OK;
    }
    BiCgStab *bi = new BiCgStab();
    int st = DPCG_OK;
    if ((st = dev_alloc(&bi->rhat, n)) < 0 || (st = dev_alloc(&bi->s, n)) < 0 || (precond_class(h) != 0 && (st = dev_alloc(&bi->sh, n)) < 0) ||
        (st = dev_alloc(&bi->t, n)) < 0 || (st = dev_alloc(&bi->part, (int64_t)kBiSlots * kMaxGrid)) < 0 ||
        (st = dev_alloc(&bi->part_rv, kMaxSpmvGrid)) < 0 || (st = dev_alloc(&bi->part_ts, kMaxSpmvGrid)) < 0 ||
        (st = dev_alloc(&bi->rec, 1)) < 0) {
        release(bi);
        return st;
    }
    h->bi = bi;
    return DPCG_OK;
}

// one update as launches on s.  The handle's vectors stand for x, r, p (h->p), v (h->q) and ph (h->z); h->t is the applies' scratch.
int enqueue_bicgstab_update(dpcg_system *h, hipStream_t s) {
    const BiCgStab *bi = h->bi;
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    const int pre = precond_class(h);
    double *ph = pre == 0 ? h->p : h->z;
    double *shv = pre == 0 ? bi->s : bi->sh;
    const dim3 grid(G), block(kBlock);
    if (pre == 0) hipLaunchKernelGGL((k_bi_pass_p<0>), grid, block, 0, s, n, h->scal, bi->rec, bi->part, G, h->r, h->p, h->q, h->dinv, ph, h->hist, h->hist_cap);
    else if (pre == 1) hipLaunchKernelGGL((k_bi_pass_p<1>), grid, block, 0, s, n, h->scal, bi->rec, bi->part, G, h->r, h->p, h->q, h->dinv, ph, h->hist, h->hist_cap);
    else hipLaunchKernelGGL((k_bi_pass_p<2>), grid, block, 0, s, n, h->scal, bi->rec, bi->part, G, h->r, h->p, h->q, h->dinv, ph, h->hist, h->hist_cap);
    if (pre == 2) DPCG_TRY(apply_precond(h, h->p, ph, s, true));                                   // ph = M p
    launch_spmv_xdot(h->A, h->planA, ph, bi->rhat, h->q, bi->part_rv, s);                           // v = A ph, <rhat,v>
    if (pre == 0) hipLaunchKernelGGL((k_bi_pass_s<0>), grid, block, 0, s, n, h->scal, bi->rec, bi->part_rv, h->planA.grid, h->r, h->q, h->dinv, bi->s, shv, bi->part);
    else if (pre == 1) hipLaunchKernelGGL((k_bi_pass_s<1>), grid, block, 0, s, n, h->scal, bi->rec, bi->part_rv, h->planA.grid, h->r, h->q, h->dinv, bi->s, shv, bi->part);
    else hipLaunchKernelGGL((k_bi_pass_s<2>), grid, block, 0, s, n, h->scal, bi->rec, bi->part_rv, h->planA.grid, h->r, h->q, h->dinv, bi->s, shv, bi->part);
    if (pre == 2) DPCG_TRY(apply_precond(h, bi->s, shv, s, true));                                 // sh = M s
    launch_spmv_xdot(h->A, h->planA, shv, bi->s, bi->t, bi->part_ts, s);                            // t = A sh, <s,t>
    hipLaunchKernelGGL(k_bi_tt, grid, block, 0, s, n, bi->rec, bi->t, bi->part);
    hipLaunchKernelGGL(k_bi_pass_x, grid, block, 0, s, n, h->scal, bi->rec, bi->part, G, bi->part_ts, h->planA.grid, h->x, ph, shv, bi->s,
                       bi->t, bi->rhat, h->r, bi->part, h->hist, h->hist_cap);
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

void free_bicgstab(dpcg_system *h) {
    release(h->bi);
    h->bi = nullptr;
}

extern "C" int dpcg_solve_bicgstab(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq, double atol_sq,
                                   int max_iter, int flags, dpcg_stream_t stream, int *iters, double *final_res, double *seconds,
                                   double *res_history) {
    if (!h || !b) return invalid("dpcg_solve_bicgstab: NULL handle or b");
    if (max_iter < 0) return invalid("dpcg_solve_bicgstab: max_iter < 0");
    if (flags & ~DPCG_NO_GRAPH) return invalid("dpcg_solve_bicgstab: flags takes 0 or DPCG_NO_GRAPH only");
    if (!std::isfinite(rtol_sq) || !std::isfinite(atol_sq)) return invalid("dpcg_solve_bicgstab: rtol_sq and atol_sq must be finite");
    if (h->ns) return invalid("dpcg_solve_bicgstab: the handle has a null space attached (the recurrence projects nothing)");
    if (h->df) return invalid("dpcg_solve_bicgstab: the handle has a deflation attached (the recurrence deflates nothing)");
    if (h->precond == DPCG_PRECOND_CALLBACK)
        return invalid("dpcg_solve_bicgstab: the callback preconditioner is not available (the driver enqueues updates ahead of the test "
                       "and a callback cannot be skipped once it has passed)");
    if (h->precond == DPCG_PRECOND_JACOBI && !h->dinv) return DPCG_ERR_STATE;
    SolveCall c{b, x0, x, rtol_sq, atol_sq, max_iter, flags, (hipStream_t)stream, iters, final_res, seconds, res_history};
    hipStream_t s = c.s;
    DPCG_TRY(ensure_bicgstab(h));
    const BiCgStab *bi = h->bi;
    const double *bp = nullptr;
    DPCG_TRY(stage_call(h, b, x0, max_iter, false, false, s, &bp));                  // x = x0 or 0;  r = b - A x
    const int G = h->vec_grid;
    hipLaunchKernelGGL(k_bi_init, dim3(G), dim3(kBlock), 0, s, h->A.n, bp, h->r, bi->rhat, h->p, h->q, bi->part);
    hipLaunchKernelGGL(k_bi_start, dim3(1), dim3(kBlock), 0, s, h->scal, bi->rec, bi->part, G, rtol_sq, atol_sq, extras()[h].prog_dev);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();
    DPCG_TRY(run_launch_ahead(h, max_iter, s, t0, " (bicgstab)", [&] { return enqueue_bicgstab_update(h, s); }));
    hipLaunchKernelGGL(k_bi_final, dim3(1), dim3(kBlock), 0, s, h->scal, bi->rec, bi->part, G, h->hist, h->hist_cap);
    return deliver_solve(h, c, t0);
}
