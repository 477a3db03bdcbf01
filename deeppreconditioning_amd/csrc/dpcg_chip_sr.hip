// Whole-solve kernel with ONE chip-wide exchange per update (DPCG_SINGLE_REDUCTION): the single-synchronisation form of CG of
// Chronopoulos and Gear (J. Comput. Appl. Math. 25, 1989; Saad's "single-synchronisation CG") in the geometry of dpcg_chip.hip's
// resident fp64 form -- hand-written for gfx950 (MI355X), M = I / Jacobi, 65 537 .. 1 048 576 rows, rows of <= 7 entries (<= 5 beyond
// 524 288 rows).
//
// k_pcg_chip keeps the reference's recurrence (cg.py:70-87), which needs two global sums an update, one after the other: <p,Ap> for
// alpha, then <r,z> for beta -- two chip-wide exchanges of about 2.7 us each in an update of 12.3 us.  This kernel multiplies A with z
// instead of p, sums <r,z>, <z,Az> and <r,r> TOGETHER and recovers q = A p from the recurrence q = A z + beta q:
//     r0 = b - A x0;  z0 = dinv o r0 (M = I: z = r);  p = q = 0;  z0 published under generation 0
//     k = 0, 1, ...:
//       s = A z_k                                  (gathered granules, row sums in CSR order)
//       gamma = <r,z>  delta = <z,s>  rho = <r,r>  (k = 0 without DPCG_INIT_CHECK_R: <z0,z0> instead of rho, the reference's first test)
//       ONE exchange; history[k] = rho / <b,b>, the test of cg.py:71; stop -> count = k; k = max_iter -> count = k, DPCG_MAX_ITER
//       beta = gamma / gamma_prev (k = 0: 0);  den = delta - (beta * gamma) / alpha_prev (k = 0: delta);  alpha = gamma / den
//       p = z + beta p;  q = s + beta q;  x += alpha p;  r -= alpha q;  z = dinv o r;  z_{k+1} published under generation k + 1
// den equals <p,Ap> in exact arithmetic.  Like k_pcg_chip's <p,Ap> it is not examined: a residual that becomes NaN ends the solve with
// DPCG_BREAKDOWN, anything else runs on to max_iter.  One product is formed after the last update before the stop is seen; x is not
// touched again.  The arithmetic differs from cg.py's, so the form is opt-in and restated by tests/single_reduction_restatement.py.
//
//   * GRANULES.  Only z travels, as SELF-VALIDATING 16-byte granules {z, z ^ key(launch, generation)} (dpcg_chip_llt.hip): a gather is
//     accepted only when its halves differ by exactly the key of the generation it wants, anything else -- the previous generation, a
//     half-written granule, the zeros the table holds at launch (every key is odd) -- is read again, within the 20 ms bound of every
//     wait here.  The gather is its own synchronisation: publishing needs no drain and no barrier, and no remote p is recomputed.
//   * ONE TABLE IS ENOUGH.  A workgroup contributes to exchange k only after its gathers of generation k are complete (delta needs
//     them), and nobody passes exchange k before all 256 have contributed.  z_{k+1} is published behind exchange k: whoever it
//     overwrites z_k for has already read it.  (x0 != 0: x0 travels the same way under a generation no update uses, and one extra
//     exchange before z_0 is published keeps it from overwriting an x0 somebody still wants.)
//   * THE EXCHANGE carries four sums (gamma, delta, rho and, at k = 0, <b,b>) as a SECOND SLOT SET IN THE SAME HOP: a second array
//     of 16-byte slots with the layout, the rotation and the re-arming of the first; the thread that stores a pair stores two, a lane
//     that polls a slot polls two -- both requests are in flight together, so a hop costs one round trip as before.  32-byte slots
//     validated as two halves would need the same two loads a lane and a second layout of the slot array besides.  The sums of both
//     sets go through the wave tree that chip::exchange2 uses, lane for lane: every workgroup adds the same values in the same
//     order (the oracle's form "chip").  exchange4 / poll_slots2 below are a copy of chip::exchange2 / poll_slots kept in step BY HAND:
//     one template over the number of sets changed the register allocation of three instantiations of this kernel and of nine elsewhere
//     ("Shared device code"), so a change to either pair must be made to both.  With M = I gamma and rho are the same
//     sum; it is carried twice rather than compiled twice.
//   * geometry, placement, visibility, co-residency: dpcg_chip.hip's (256 x 512 threads, rows v * per + t + 512 k, values in LDS and
//     registers, 16-bit column offsets, XCD reporting, the plain copy inside a group and the written-through copy for the rows within
//     the band of a group's edge, bounded waits, DPCG_ERR_STATE -> the caller's multi-launch path with the standard recurrence).
//   * REGISTERS.  s lives across the exchange beside x, r, p, q and dinv; at 8 rows a thread x moves to memory (XMEM: the thread's own
//     rows of a work vector, read and written once an update) -- see DESIGN section 3 for the register table.
#include <algorithm>

#include "dpcg_chip_device.h"

namespace dpcg {

using namespace chip;

namespace {

// polls two slots per lane (one of each set; lanes < count of wave 0) until none is pending; false when the wait ran out
__device__ __forceinline__ bool poll_slots2(const Exchange &X, const __amdgpu_buffer_rsrc_t &part2_rs, u32x4 &sa, u32x4 &sb, int off, int count) {
    const int t = threadIdx.x;
    const bool mine = t < count;
    sa = pack_f64x2(0.0, 0.0);
    sb = pack_f64x2(0.0, 0.0);
    if (mine) {
        sa = __builtin_amdgcn_raw_buffer_load_b128(X.part_rs, off, 0, kSc1);
        sb = __builtin_amdgcn_raw_buffer_load_b128(part2_rs, off, 0, kSc1);
    }
    BoundedWait wait;
    while (__ballot(mine && (is_pending(sa) || is_pending(sb))) != 0) {
        __builtin_amdgcn_s_sleep(1);
        if (mine && is_pending(sa)) sa = __builtin_amdgcn_raw_buffer_load_b128(X.part_rs, off, 0, kSc1);
        if (mine && is_pending(sb)) sb = __builtin_amdgcn_raw_buffer_load_b128(part2_rs, off, 0, kSc1);
        if (wait.give_up(X.err)) return false;
    }
    return true;
}

// chip::exchange2 with a second slot set (part2_rs: kChipSlotBytes, preset to the pending pattern like the first): four chip-wide sums
// at once and a chip barrier in the same breath.  Generation and LDS phase are X's, so it may follow exchange2 calls on the same X;
// once it has run, every later exchange of the launch must be this one (the second set is re-armed only here).
// sh4: 2 x 32 doubles of LDS, s_res4: 2 x 4.
__device__ __forceinline__ bool exchange4(Exchange &X, const __amdgpu_buffer_rsrc_t &part2_rs, double *sh4, double (*s_res4)[4], const double (&in)[4],
                                          double (&out)[4]) {
    const int t = threadIdx.x;
    double *slot = sh4 + (X.sum_phase & 1) * 32;
    ++X.sum_phase;
    double w4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = wave_sum(in[i]);
    if ((t & 63) == 63) {
#pragma unroll
        for (int i = 0; i < 4; ++i) slot[8 * i + (t >> 6)] = w4[i];
    }
    __syncthreads();
    const int set_cur = (int)(X.gen & 3u), set_nxt = (int)((X.gen + 2u) & 3u);
    double *const sres = s_res4[X.gen & 1u];
    ++X.gen;
    if (t < 64) {                                              // wave 0 does the exchange
        const unsigned plo = (unsigned)(kChipPending & 0xffffffffu), phi = (unsigned)(kChipPending >> 32);
        u32x4 pend;
        pend.x = plo; pend.y = phi; pend.z = plo; pend.w = phi;
        // hop 1: the group's 32 quadruples
        if (t == 0) {
            double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int w = 0; w < kChipThreads / 64; ++w) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s4[i] += slot[8 * i + w];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-arm of the previous generation has landed
            const int o_n = (set_nxt * kChipWGs + X.v) * 16, o_c = (set_cur * kChipWGs + X.v) * 16;
            if (X.local) {
                __builtin_amdgcn_raw_buffer_store_b128(pend, X.part_rs, o_n, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(pend, part2_rs, o_n, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(s4[0], s4[1]), X.part_rs, o_c, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(s4[2], s4[3]), part2_rs, o_c, 0, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b128(pend, X.part_rs, o_n, 0, kSc1);
                __builtin_amdgcn_raw_buffer_store_b128(pend, part2_rs, o_n, 0, kSc1);
                __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(s4[0], s4[1]), X.part_rs, o_c, 0, kSc1);
                __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(s4[2], s4[3]), part2_rs, o_c, 0, kSc1);
            }
        }
        u32x4 sa, sb;
        int ok = poll_slots2(X, part2_rs, sa, sb, (set_cur * kChipWGs + X.grp * 32 + t) * 16, 32) ? 1 : 0;
        const double g0 = wave_sum(lo_f64(sa)), g1 = wave_sum(hi_f64(sa));      // (lanes 32-63 add +0.0)
        const double g2 = wave_sum(lo_f64(sb)), g3 = wave_sum(hi_f64(sb));
        // hop 2: eight members of the group hand its quadruple to the eight groups, everybody sums the eight of its group's line
        if (t == 63 && X.rank < 8) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int o_n = kChipS1Bytes + ((set_nxt * 8 + X.rank) * 8 + X.grp) * 16, o_c = kChipS1Bytes + ((set_cur * 8 + X.rank) * 8 + X.grp) * 16;
            __builtin_amdgcn_raw_buffer_store_b128(pend, X.part_rs, o_n, 0, kSc1);
            __builtin_amdgcn_raw_buffer_store_b128(pend, part2_rs, o_n, 0, kSc1);
            __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(g0, g1), X.part_rs, o_c, 0, kSc1);
            __builtin_amdgcn_raw_buffer_store_b128(pack_f64x2(g2, g3), part2_rs, o_c, 0, kSc1);
        }
        if (ok) ok = poll_slots2(X, part2_rs, sa, sb, kChipS1Bytes + ((set_cur * 8 + X.grp) * 8 + t) * 16, 8) ? 1 : 0;
        const double t0 = wave_sum(lo_f64(sa)), t1 = wave_sum(hi_f64(sa));      // (lanes 8-63 add +0.0)
        const double t2 = wave_sum(lo_f64(sb)), t3 = wave_sum(hi_f64(sb));
        if (t == 63) {
            sres[0] = t0; sres[1] = t1; sres[2] = t2; sres[3] = t3;
            *X.s_flag = ok;
        }
    }
    __syncthreads();
    if (!*X.s_flag) return false;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = sres[i];
    return true;       // (sres is written again two exchanges on, behind the barriers of the next one)
}

constexpr unsigned kGenX0 = 0xffffffffu;    // the generation x0 travels under: no update reaches it (max_iter < 2^31)

// RPT: rows per thread (2, 4, 8); WMAX: entry slots per row (5, 7; 5 at 8 rows a thread); JAC: M = diag(1 / a_ii) (else M = I); XMEM: x of the own rows in
// memory (d.xwork) instead of registers.
template <int RPT, int WMAX, bool JAC, bool XMEM>
__global__ __launch_bounds__(kChipThreads) void k_pcg_chip_sr(const ChipSrDesc ds) {
    const ChipDesc &d = ds.c;
    constexpr int NS = RPT * WMAX;                                   // entry slots of a thread
    constexpr int NLDS = NS < kChipLdsSlots ? NS : kChipLdsSlots;    // ... whose values live in LDS
    constexpr int NREG = NS - NLDS;                                  // ... and in registers (the first NREG slots)
    extern __shared__ __attribute__((aligned(16))) double chip_lv[];   // [NLDS][512]: slot s of thread t at [(s - NREG) * 512 + t]
    __shared__ double sh[2 * 16];          // chip::exchange2 (the XCD report)
    __shared__ double s_res[2][2];
    __shared__ double sh4[2 * 32];         // exchange4: block sums, two halves in turn, 4 x 8 wave sums each
    __shared__ double s_res4[2][4];        // the reduced quadruple, two sets in turn
    __shared__ int s_flag;
    const int t = threadIdx.x;
    const int v = ((int)blockIdx.x & 7) * (kChipWGs / 8) + ((int)blockIdx.x >> 3);
    const int row0 = v * d.per + t;        // row of slot k: row0 + 512 k
    const int grp = (int)blockIdx.x & 7, rank = (int)blockIdx.x >> 3;       // v = 32 grp + rank
    const int glo = grp * (kChipWGs / 8) * d.per;                           // the group's rows: [glo, ghi)
    const int ghi = (glo + (kChipWGs / 8) * d.per < d.n) ? glo + (kChipWGs / 8) * d.per : d.n;
    const int remote_base = (d.n + kChipZpPad) * 16;
    const __amdgpu_buffer_rsrc_t zp_rs = chip_rsrc(d.zp, 2u * (unsigned)(d.n + kChipZpPad) * 16u);
    const __amdgpu_buffer_rsrc_t part2_rs = chip_rsrc(ds.part2, (unsigned)kChipSlotBytes);

    // ---- the matrix slice and the vectors of the own rows: read once (as k_pcg_chip does) ----------------------------------
    double vr[NREG > 0 ? NREG : 1];
    unsigned dl[(NS + 1) / 2];
    unsigned lens = 0;                      // four bits per row: the top one = the row exists, below it the length
    double x[XMEM ? 1 : RPT], r[RPT], p[RPT], q[RPT], s[RPT], dv[JAC ? RPT : 1];
    double bb_loc = 0.0;
    int rs_k[RPT], len_k[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int loc = k * kChipThreads + t, i = row0 + k * kChipThreads;
        const bool valid = loc < d.per && i < d.n;
        const int ic = valid ? i : 0;
        const int rs = d.rp[ic], re = d.rp[ic + 1];
        const double bi = d.b[ic];
        const double xi = d.x0 ? d.x0[ic] : 0.0;
        const double di = JAC ? d.dinv[ic] : 1.0;
        rs_k[k] = rs;
        len_k[k] = valid ? re - rs : 0;
        lens |= (valid ? (8u | (unsigned)(re - rs)) : 0u) << (4 * k);
        if (XMEM) { if (valid) ds.xwork[i] = xi; }
        else x[XMEM ? 0 : k] = valid ? xi : 0.0;
        r[k] = valid ? bi : 0.0;
        p[k] = q[k] = s[k] = 0.0;
        if (JAC) dv[k] = valid ? di : 1.0;
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        if (row_valid_bits(lens, k)) bb_loc += r[k] * r[k];
        const int i = row0 + k * kChipThreads;
        int cj[WMAX];
        double aj[WMAX];
#pragma unroll
        for (int j = 0; j < WMAX; ++j) {
            const int e = j < len_k[k] ? rs_k[k] + j : 0;          // (entry 0 exists: nnz >= n >= 1)
            cj[j] = d.ci[e];
            aj[j] = d.val[e];
        }
#pragma unroll
        for (int j = 0; j < WMAX; ++j) {
            const bool on = j < len_k[k];
            put_slot<NREG>(k * WMAX + j, i, on ? cj[j] : i, on ? aj[j] : 0.0, dl, vr, chip_lv + t);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    bool local = false;                     // every group on one XCD (established below, once per solve)
    auto row_on = [&](int k) -> bool { return row_valid_bits(lens, k); };

    // s = A z for the own rows out of the granules of generation `gen`; a row whose granules are not all of that generation yet is
    // gathered again.  The next row's gathers are issued while this row's are checked and consumed; row sums in CSR order.
    // Returns false (for the whole workgroup) when a wait ran out.
    auto spmv = [&](unsigned gen) -> bool {
        u32x4 g[2][WMAX];
        // (opaque copies per call: the LDS reads, the gather addresses and the lane masks are loop-invariant, and hoisted out of the
        // update loop they would take registers the kernel does not have -- see dpcg_chip.hip)
        int tl = t;
        asm volatile("" : "+v"(tl));
        const double *lvt = chip_lv + tl;
        int glo_l = glo, span_l = local ? ghi - glo : 0;
        const int local_shift = grp * 128;
        asm volatile("" : "+s"(glo_l), "+s"(span_l));
#pragma unroll
        for (int e = 0; e < (NS + 1) / 2; ++e) asm volatile("" : "+v"(dl[e]));
        asm volatile("" : "+v"(lens));
        const unsigned long long key = granule_key(ds.nonce, gen);
        const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
        auto address = [&](int k, int j) -> int {
            const int sl = k * WMAX + j;
            const int del = (int)((dl[sl >> 1] >> (16 * (sl & 1))) & 0xffffu);
            const int c = row0 + k * kChipThreads + del - 32768;
            const bool own = (unsigned)(c - glo_l) < (unsigned)span_l;              // the column's owner is in this group: the plain copy
            return c * 16 + (own ? local_shift : remote_base);
        };
        auto request = [&](int k, u32x4 (&gk)[WMAX]) {
#pragma unroll
            for (int j = 0; j < WMAX; ++j) gk[j] = __builtin_amdgcn_raw_buffer_load_b128(zp_rs, address(k, j), 0, kSc1);
        };
        bool ok = true;
        request(0, g[0]);
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k + 1 < RPT) request(k + 1, g[(k + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);                     // (two rows' granules in flight is what the registers hold)
            const int len = (int)((lens >> (4 * k)) & 7u);
            BoundedWait wait;
            for (;;) {
                bool bad = false;
#pragma unroll
                for (int j = 0; j < WMAX; ++j) bad = bad || (j < len && ((g[k & 1][j].x ^ g[k & 1][j].z) != klo || (g[k & 1][j].y ^ g[k & 1][j].w) != khi));
                if (__ballot(bad) == 0) break;
                __builtin_amdgcn_s_sleep(1);
                if (bad) request(k, g[k & 1]);                     // (the whole row again: one divergent region)
                if (wait.give_up(d.err)) {
                    ok = false;
                    break;
                }
            }
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < WMAX; ++j) {
                const int sl = k * WMAX + j;
                const double a = sl < NREG ? vr[sl < NREG ? sl : 0] : lvt[(sl - NREG) * kChipThreads];
                if (j < len) acc += a * lo_f64(g[k & 1][j]);
            }
            s[k] = acc;
            __builtin_amdgcn_sched_barrier(0);
        }
        return __syncthreads_and(ok ? 1 : 0) != 0;
    };

    Exchange X = make_exchange(d.part, v, grp, rank, sh, s_res, &s_flag, d.err);
    unsigned far_rows = 0xffu;              // bit k: row k of this thread is gathered by another group (all of them until `local` holds)
    int row0_l = row0;                      // an opaque copy per update: hoisted store addresses are registers the loop does not have
    auto publish = [&](int k, double zk, unsigned long long key) {
        const int o = (row0_l + k * kChipThreads) * 16;
        const u32x4 w = tagged_granule(zk, key);
        store_granule(w, zp_rs, o, grp, remote_base, local, ((far_rows >> k) & 1u) != 0);
    };

    bool alive = true;
    // ---- where the groups sit: every workgroup reports its XCD, everybody reads the 256 answers ---------------------------
    if (d.xcc) local = place_groups<RPT>(X, d.xcc, row0, glo, ghi, d.band, far_rows, alive);
    const double zero4[4] = {0.0, 0.0, 0.0, 0.0};
    double sum4[4] = {0.0, 0.0, 0.0, 0.0};
    // ---- r0 = b - A x0 ---------------------------------------------------------------------------------------------------
    if (alive && d.x0) {
        const unsigned long long key_x0 = granule_key(ds.nonce, kGenX0);
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (row_on(k)) publish(k, XMEM ? ds.xwork[row0 + k * kChipThreads] : x[XMEM ? 0 : k], key_x0);
        alive = spmv(kGenX0);
#pragma unroll
        for (int k = 0; k < RPT; ++k) r[k] = r[k] - s[k];
        if (alive) alive = exchange4(X, part2_rs, sh4, s_res4, zero4, sum4);   // everybody has read x0 out of the granules before z_0 overwrites them
    }
    {
        const unsigned long long key0 = granule_key(ds.nonce, 0u);
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (alive && row_on(k)) publish(k, JAC ? dv[JAC ? k : 0] * r[k] : r[k], key0);
    }
    double bb = 0.0, res = 0.0, gamma_prev = 1.0, alpha_prev = 1.0;
    int k_done = 0, status = DPCG_MAX_ITER;
    // ---- the updates: one chip-wide exchange each ----------------------------------------------------------------------------
    while (alive) {
        if (!(alive = spmv((unsigned)k_done))) break;              // s = A z_k
        double in4[4] = {0.0, 0.0, 0.0, 0.0};
        const bool first_on_z = k_done == 0 && !d.init_check_r;    // cg.py:66: the first test is on z
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const double zk = JAC ? dv[JAC ? k : 0] * r[k] : r[k];
            if (row_on(k)) {
                in4[0] += r[k] * zk;
                in4[1] += zk * s[k];
                in4[2] += first_on_z ? zk * zk : r[k] * r[k];
            }
        }
        in4[3] = k_done == 0 ? bb_loc : 0.0;
        if (!(alive = exchange4(X, part2_rs, sh4, s_res4, in4, sum4))) break;
        const double gamma = sum4[0], delta = sum4[1], rho = sum4[2];
        if (k_done == 0) bb = sum4[3];
        res = rho / bb;                                            // cg.py:86 (k = 0: cg.py:66)
        if (v == 0 && t == 0 && k_done < d.hist_cap) d.hist[k_done] = res;
        const bool conv = (res < d.rtol_sq) || (rho < d.atol_sq);  // cg.py:71
        if (conv) { status = DPCG_OK; break; }
        if (!(res == res)) { status = DPCG_BREAKDOWN; break; }
        if (k_done >= d.max_iter) break;
        const double beta = k_done == 0 ? 0.0 : gamma / gamma_prev;
        const double den = k_done == 0 ? delta : delta - (beta * gamma) / alpha_prev;
        const double alpha = gamma / den;
        gamma_prev = gamma;
        alpha_prev = alpha;
        ++k_done;
        const unsigned long long key = granule_key(ds.nonce, (unsigned)k_done);
        asm volatile("" : "+v"(row0_l), "+v"(far_rows));
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const double zk = JAC ? dv[JAC ? k : 0] * r[k] : r[k];
            p[k] = zk + beta * p[k];
            q[k] = s[k] + beta * q[k];
            if (XMEM) {
                if (row_on(k)) {
                    double *xp = ds.xwork + (row0_l + k * kChipThreads);
                    *xp = *xp + alpha * p[k];
                }
            } else {
                x[XMEM ? 0 : k] = x[XMEM ? 0 : k] + alpha * p[k];
            }
            r[k] = r[k] - alpha * q[k];
            if (row_on(k)) publish(k, JAC ? dv[JAC ? k : 0] * r[k] : r[k], key);
        }
    }
    // (after a wait that ran out the workgroups are not at the same update: nothing is stored -- see dpcg_chip.hip)
#pragma unroll
    for (int k = 0; k < RPT; ++k)
        if (alive && row_on(k)) {
            const int i = row0 + k * kChipThreads;
            if (XMEM) { if (d.x != ds.xwork) d.x[i] = ds.xwork[i]; }
            else d.x[i] = x[XMEM ? 0 : k];
        }
    if (v == 0 && t == 0) {
        store_scalars(d.out, k_done, res, bb, alive, status);
    }
}

template <int RPT, int WMAX, bool JAC, bool XMEM>
int chip_sr_launch(const ChipSrDesc &ds, hipStream_t s, bool check_only) {
    constexpr int NS = RPT * WMAX;
    constexpr int NLDS = NS < kChipLdsSlots ? NS : kChipLdsSlots;
    const int lds = NLDS * kChipThreads * (int)sizeof(double);
    return chip_launch_resident<k_pcg_chip_sr<RPT, WMAX, JAC, XMEM>>(lds, ds, s, check_only);
}

}  // namespace

// rows of up to 7 entries while a thread holds at most four rows (524 288 rows), 5 beyond: eight rows of 7 entries spill with x in
// memory too
int chip_sr_max_row_len(int64_t n) { return n <= (int64_t)kChipWGs * kChipThreads * 4 ? 7 : 5; }

// One system on the whole chip with the single-reduction recurrence.  max_row_len <= chip_sr_max_row_len(n); d.per = ceil(n / 256) <= 4096.
// Returns DPCG_OK, DPCG_ERR_STATE when the kernel cannot be resident on every CU, or a negative status.
int launch_pcg_chip_sr(const ChipSrDesc &ds, int max_row_len, hipStream_t s, bool check_only) {
    const ChipDesc &d = ds.c;
    const int rpt = (d.per + kChipThreads - 1) / kChipThreads;
    const bool jac = d.precond == DPCG_PRECOND_JACOBI;
    if (max_row_len < 1 || max_row_len > chip_sr_max_row_len(d.n) || d.per < 1 || d.per > kChipThreads * kChipMaxRpt) return DPCG_ERR_INVALID;
    if (d.f32 || d.stream_cap || d.bench || d.dbg || !ds.part2 || !ds.xwork || ds.nonce == 0) return DPCG_ERR_INVALID;
#define DPCG_SR_W(RPTV, WV, XM) (jac ? chip_sr_launch<RPTV, WV, true, XM>(ds, s, check_only) : chip_sr_launch<RPTV, WV, false, XM>(ds, s, check_only))
#define DPCG_SR_R(RPTV, XM) (max_row_len <= 5 ? DPCG_SR_W(RPTV, 5, XM) : DPCG_SR_W(RPTV, 7, XM))
    if (rpt <= 2) return DPCG_SR_R(2, false);
    if (rpt <= 4) return DPCG_SR_R(4, false);
    return DPCG_SR_W(8, 5, true);
#undef DPCG_SR_R
#undef DPCG_SR_W
}

}  // namespace dpcg
