// Saad's dual-threshold ILUT(p, tau): the device routine behind dpcg_set_precond_ilut (contract: tests/ilut_restatement.py; it
// replaces `ilupp.ilut(matrix)`, the reference harness's `incomplete_lu` technique, test.py:90-93).  Row by row, in the caller's
// numbering: w = A[i, :]; tau_i = threshold * ||A[i, :]||_2; for the columns k < i of w in ascending order (fill included)
// w_k /= U_kk, dropped when |w_k| < tau_i, else w_j -= w_k U_kj for the kept U[k, j > k]; of the surviving L part the
// nnz(A[i, :i]) + add_fill_in largest stay, of the U part those >= tau_i and of them the nnz(A[i, i+1:]) + add_fill_in largest
// (ties: the smaller column); U_ii = w_i, L_ii = 1.
//
// Which fill survives depends on the VALUES of the rows before, so -- as for icholt's columns (dpcg_icholt.hip) -- there is no
// symbolic phase to build level sets from: the factorisation is a sequence of n small steps, walked by ONE wave.  The 64 lanes
// share row i: its candidates live in registers, kIlutSlots per lane (slot s of lane l: candidate 64 s + l, up to 256 positions);
// the next k is a wave-wide minimum; w -= w_k U[k, :] matches each entry of U row k to its candidate by a compare across the wave
// (a miss appends a fill candidate); the two selections count ranks across the wave.  Every sum in the restatement's order (one
// product and one subtraction at a time; -ffp-contract=off), so L and U equal the restatement bit for bit.
//
// Memory: the kept rows of U go to per-row lists (kIlutCap entries each) that later rows read; L's rows go to lists of their own
// (nothing reads them until the CSR is emitted).  At the start of a row the U rows of the first kIlutPre L-part columns A's own
// pattern names are requested together, and row i + 1 of A is fetched while row i is worked on: only a k that fill created costs a
// dependent round trip of its own.  One wave's vector-memory operations reach its CU's L1 in order, so a row stored by the wave is
// there for the wave's later loads with wavefront-scope ordering only (as in dpcg_icholt.hip).
#include "dpcg_host.h"
#include "dpcg_prims.h"

namespace dpcg {
namespace {

constexpr int kIlutCap = 64;                  // kept entries per row of L and per row of U, diagonals aside (beyond: DPCG_ERR_INVALID)
constexpr int kIlutSlots = 4;                 // candidates per lane
constexpr int kIlutCand = 64 * kIlutSlots;    // positions one working row may hold (beyond: DPCG_ERR_INVALID)
constexpr int kIlutPre = 4;                   // U rows requested at the start of a row

enum { ILUT_OK = 0, ILUT_PIVOT = 1, ILUT_CAND = 2, ILUT_CAP = 3 };

__device__ __forceinline__ int ld_i(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ double ld_d(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void st_i(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void st_d(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double lane_d(double v, int l) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int first_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return first_i(v);
}
// slot s of a per-lane array, read from lane l (s, l the same for every lane): every slot is read and the reads are selected
// between, so the arrays stay in registers (a select between loads of an array would turn into an indexed load: scratch)
__device__ __forceinline__ int lane_pick_i(const int (&a)[kIlutSlots], int s, int l) {
    int r = lane_i(a[0], l);
#pragma unroll
    for (int t = 1; t < kIlutSlots; ++t) { const int v = lane_i(a[t], l); r = s == t ? v : r; }
    return r;
}
__device__ __forceinline__ double lane_pick_d(const double (&a)[kIlutSlots], int s, int l) {
    double r = lane_d(a[0], l);
#pragma unroll
    for (int t = 1; t < kIlutSlots; ++t) { const double v = lane_d(a[t], l); r = s == t ? v : r; }
    return r;
}
__device__ __forceinline__ bool bit_of(const unsigned long long (&b)[kIlutSlots], int s, int l) {
    unsigned long long r = 0ull;
#pragma unroll
    for (int t = 0; t < kIlutSlots; ++t) r |= s == t ? b[t] : 0ull;
    return (r >> l) & 1ull;
}

// Of the candidates `e` (slot-wise), keep the p largest |w| (ties: the smaller column); pos = rank of a kept one by column.
// nl: candidates in use (slots beyond hold kNone / 0).  Returns the number kept.
__device__ __forceinline__ int select_largest(const bool (&e)[kIlutSlots], const int (&col)[kIlutSlots], const double (&mag)[kIlutSlots],
                                              int nl, int p, bool (&keep)[kIlutSlots], int (&pos)[kIlutSlots]) {
    unsigned long long eb[kIlutSlots];
    int count = 0;
#pragma unroll
    for (int s = 0; s < kIlutSlots; ++s) {
        eb[s] = __ballot(e[s]);
        count += __popcll(eb[s]);
        keep[s] = e[s];
    }
    if (count > p) {
        int better[kIlutSlots] = {};
        for (int o = 0; o < nl; ++o) {
            const int os = o >> 6, ol = o & 63;
            if (!bit_of(eb, os, ol)) continue;
            const double om = lane_pick_d(mag, os, ol);
            const int oc = lane_pick_i(col, os, ol);
#pragma unroll
            for (int s = 0; s < kIlutSlots; ++s) better[s] += (om > mag[s] || (om == mag[s] && oc < col[s])) ? 1 : 0;
        }
#pragma unroll
        for (int s = 0; s < kIlutSlots; ++s) keep[s] = e[s] && better[s] < p;
    }
    unsigned long long kb[kIlutSlots];
    int kept = 0;
#pragma unroll
    for (int s = 0; s < kIlutSlots; ++s) {
        kb[s] = __ballot(keep[s]);
        kept += __popcll(kb[s]);
        pos[s] = 0;
    }
    if (kept > kIlutCap) return kept;
    for (int o = 0; o < nl; ++o) {
        const int os = o >> 6, ol = o & 63;
        if (!bit_of(kb, os, ol)) continue;
        const int oc = lane_pick_i(col, os, ol);
#pragma unroll
        for (int s = 0; s < kIlutSlots; ++s) pos[s] += oc < col[s] ? 1 : 0;
    }
    return kept;
}

// lcnt / ucnt[i]: kept entries of row i of L / U (diagonals aside); the entries at [i * kIlutCap ..], columns ascending; udiag[i] = U_ii.
// status[0] = code, status[1] = row.
__global__ __launch_bounds__(64) void k_ilut(int n, const int32_t *__restrict__ arp, const int32_t *__restrict__ aci,
                                             const double *__restrict__ av, int add_fill, double threshold, int *lcnt, int *lcol,
                                             double *lval, int *ucnt, int *ucol, double *uval, double *udiag, int *status) {
    constexpr int kNone = 0x7fffffff;
    constexpr int S = kIlutSlots;
    const int lane = threadIdx.x;
    // row r of A into the slots (entries in ascending column: slot order is column order)
    auto fetch_row = [&](int r, int &na, int (&c)[S], double (&v)[S]) {
        const int a0 = arp[r], a1 = arp[r + 1];
        na = a1 - a0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int q = s * 64 + lane;
            c[s] = q < na ? aci[a0 + q] : kNone;
            v[s] = q < na ? av[a0 + q] : 0.0;
        }
    };
    int na = 0, ncol[S];
    double nval[S];
    fetch_row(0, na, ncol, nval);
    for (int i = 0; i < n; ++i) {
        int col[S], st[S];                            // st: 0 open, 1 kept, 2 dropped (columns < i)
        double val[S];
#pragma unroll
        for (int s = 0; s < S; ++s) { col[s] = ncol[s]; val[s] = nval[s]; st[s] = 0; }
        const int na_i = na;
        if (i + 1 < n) fetch_row(i + 1, na, ncol, nval);      // (fetched ahead: A is read-only)
        if (na_i > kIlutCand) {
            if (lane == 0) { status[0] = ILUT_CAND; status[1] = i; }
            return;
        }
        // ---- tau_i from the original row (squares in ascending column), the two count bounds
        double sq[S];
#pragma unroll
        for (int s = 0; s < S; ++s) sq[s] = val[s] * val[s];
        double ss = 0.0;
        for (int c = 0; c < na_i; ++c) ss = ss + lane_pick_d(sq, c >> 6, c & 63);
        const double tau = threshold * sqrt(ss);
        int n_lo = 0, n_up = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            n_lo += __popcll(__ballot(col[s] < i));
            n_up += __popcll(__ballot(col[s] > i && col[s] != kNone));
        }
        const int p_lo = n_lo + add_fill, p_up = n_up + add_fill;
        // ---- U rows of A's first L-part columns (slots 0 .. n_lo - 1), requested together
        int pk[kIlutPre], pc[kIlutPre], pn[kIlutPre];
        double pv[kIlutPre], pd[kIlutPre];
#pragma unroll
        for (int t = 0; t < kIlutPre; ++t) {
            pk[t] = t < n_lo ? lane_i(col[0], t) : -1;
            pc[t] = 0; pn[t] = 0; pv[t] = 0.0; pd[t] = 1.0;
            if (pk[t] >= 0) {
                pc[t] = ld_i(ucol + (size_t)pk[t] * kIlutCap + lane);
                pv[t] = ld_d(uval + (size_t)pk[t] * kIlutCap + lane);
                pd[t] = ld_d(udiag + pk[t]);
                pn[t] = ld_i(ucnt + pk[t]);
            }
        }
        int nl = na_i;
        // ---- the eliminations, k ascending
        for (;;) {
            int mk = kNone;
#pragma unroll
            for (int s = 0; s < S; ++s) mk = (col[s] < i && st[s] == 0 && col[s] < mk) ? col[s] : mk;
            const int k = wave_min(mk);
            if (k == kNone) break;
            int ks = 0, kl = 0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const unsigned long long b = __ballot(col[s] == k);
                if (b) { ks = s; kl = __ffsll((long long)b) - 1; }
            }
            int uc = 0, um = 0;
            double uv = 0.0, ud = 1.0;
            bool have = false;
#pragma unroll
            for (int t = 0; t < kIlutPre; ++t)
                if (pk[t] == k) { uc = pc[t]; uv = pv[t]; ud = pd[t]; um = pn[t]; have = true; }
            if (!have) {                              // (a column that fill created: its own round trip)
                uc = ld_i(ucol + (size_t)k * kIlutCap + lane);
                uv = ld_d(uval + (size_t)k * kIlutCap + lane);
                ud = ld_d(udiag + k);
                um = ld_i(ucnt + k);
            }
            const double wk = lane_pick_d(val, ks, kl) / ud;
            const bool drop = fabs(wk) < tau;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (s == ks && lane == kl) { val[s] = wk; st[s] = drop ? 2 : 1; }
            if (drop) continue;
            um = first_i(um);
            for (int q = 0; q < um; ++q) {
                const int j = lane_i(uc, q);
                const double prod = wk * lane_d(uv, q);
                bool hit = false;
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (col[s] == j) { val[s] = val[s] - prod; hit = true; }
                if (!__ballot(hit)) {                 // fill: a new candidate
                    if (nl >= kIlutCand) {
                        if (lane == 0) { status[0] = ILUT_CAND; status[1] = i; }
                        return;
                    }
                    const int ts = nl >> 6, tl = nl & 63;
#pragma unroll
                    for (int s = 0; s < S; ++s)
                        if (s == ts && lane == tl) { col[s] = j; val[s] = 0.0 - prod; st[s] = 0; }
                    ++nl;
                }
            }
        }
        // ---- the pivot
        double wi = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const unsigned long long b = __ballot(col[s] == i);
            if (b) wi = lane_d(val[s], __ffsll((long long)b) - 1);
        }
        if (!(wi != 0.0) || !__builtin_isfinite(wi)) {
            if (lane == 0) { status[0] = ILUT_PIVOT; status[1] = i; }
            return;
        }
        // ---- the two selections
        bool el[S], eu[S], kl_[S], ku[S];
        int pl[S], pu[S];
        double mag[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            mag[s] = fabs(val[s]);
            el[s] = col[s] < i && st[s] == 1;
            eu[s] = col[s] > i && col[s] != kNone && !(mag[s] < tau);
        }
        const int nkl = select_largest(el, col, mag, nl, p_lo, kl_, pl);
        const int nku = select_largest(eu, col, mag, nl, p_up, ku, pu);
        if (nkl > kIlutCap || nku > kIlutCap) {
            if (lane == 0) { status[0] = ILUT_CAP; status[1] = i; }
            return;
        }
        // ---- row i of L and of U into their lists
        const size_t base = (size_t)i * kIlutCap;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (kl_[s]) { st_i(lcol + base + pl[s], col[s]); st_d(lval + base + pl[s], val[s]); }
            if (ku[s]) { st_i(ucol + base + pu[s], col[s]); st_d(uval + base + pu[s], val[s]); }
        }
        if (lane == 0) {
            st_i(lcnt + i, nkl);
            st_i(ucnt + i, nku);
            st_d(udiag + i, wi);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// L as CSR (row i: its list, then the unit diagonal) and U (row i: the diagonal, then its list)
__global__ __launch_bounds__(kBlock) void k_ilut_count(int n, const int *__restrict__ lcnt, const int *__restrict__ ucnt,
                                                       int32_t *__restrict__ cl, int32_t *__restrict__ cu) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) { cl[i] = lcnt[i] + 1; cu[i] = ucnt[i] + 1; }
    if (i == n) { cl[i] = 0; cu[i] = 0; }
}
__global__ __launch_bounds__(kBlock) void k_ilut_emit(int n, const int *__restrict__ lcnt, const int *__restrict__ lcol,
                                                      const double *__restrict__ lval, const int *__restrict__ ucnt,
                                                      const int *__restrict__ ucol, const double *__restrict__ uval,
                                                      const double *__restrict__ udiag, const int32_t *__restrict__ lrp,
                                                      int32_t *__restrict__ lci, double *__restrict__ lv, const int32_t *__restrict__ urp,
                                                      int32_t *__restrict__ uci, double *__restrict__ uv) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)i * kIlutCap;
    const int ml = lcnt[i], la = lrp[i];
    for (int q = 0; q < ml; ++q) {
        lci[la + q] = lcol[base + q];
        lv[la + q] = lval[base + q];
    }
    lci[la + ml] = i;
    lv[la + ml] = 1.0;
    const int mu = ucnt[i], ua = urp[i];
    uci[ua] = i;
    uv[ua] = udiag[i];
    for (int q = 0; q < mu; ++q) {
        uci[ua + 1 + q] = ucol[base + q];
        uv[ua + 1 + q] = uval[base + q];
    }
}

}  // namespace
}  // namespace dpcg

// Factor `A` (the caller's matrix: CSR with sorted columns) into Lf (unit lower, diagonal last) and Uf (upper, diagonal first),
// both owned.  Leaves both empty on failure.
int ilut_factor(const CsrDev &A, int add_fill_in, double threshold, CsrDev &Lf, CsrDev &Uf, hipStream_t s) {
    const int64_t n = A.n;
    if (n > 0x7fffffff / kIlutCap) return invalid("dpcg_set_precond_ilut: too many rows for the per-row lists");
    int *lcnt = nullptr, *lcol = nullptr, *ucnt = nullptr, *ucol = nullptr, *status = nullptr;
    int32_t *cl = nullptr, *cu = nullptr;
    double *lval = nullptr, *uval = nullptr, *udiag = nullptr;
    Lf = CsrDev{};
    Uf = CsrDev{};
    Lf.n = Uf.n = n;
    Lf.owned = Uf.owned = true;
    auto cleanup = [&](int st) {
        dev_free(lcnt); dev_free(lcol); dev_free(ucnt); dev_free(ucol); dev_free(status); dev_free(cl); dev_free(cu);
        dev_free(lval); dev_free(uval); dev_free(udiag);
        if (st < 0) { free_csr(Lf); free_csr(Uf); }
        return st;
    };
    int st = DPCG_OK;
    const int64_t wide = n * kIlutCap;
    if ((st = dev_alloc(&lcnt, n)) < 0 || (st = dev_alloc(&lcol, wide)) < 0 || (st = dev_alloc(&lval, wide)) < 0 ||
        (st = dev_alloc(&ucnt, n)) < 0 || (st = dev_alloc(&ucol, wide)) < 0 || (st = dev_alloc(&uval, wide)) < 0 ||
        (st = dev_alloc(&udiag, n)) < 0 || (st = dev_alloc(&status, 2)) < 0 || (st = dev_alloc(&cl, n + 1)) < 0 ||
        (st = dev_alloc(&cu, n + 1)) < 0 || (st = dev_alloc(&Lf.rowptr, n + 1)) < 0 || (st = dev_alloc(&Uf.rowptr, n + 1)) < 0)
        return cleanup(st);
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int), s);
    if (e != hipSuccess) return cleanup(hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__));
    hipLaunchKernelGGL(k_ilut, dim3(1), dim3(64), 0, s, (int)n, A.rowptr, A.col, A.val, add_fill_in, threshold, lcnt, lcol, lval,
                       ucnt, ucol, uval, udiag, status);
    int h_status[2] = {0, 0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_status, status, sizeof(h_status), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return cleanup(hip_fail(e, "ilut", __FILE__, __LINE__));
    if (h_status[0] != ILUT_OK) {
        const std::string at = " at row " + std::to_string(h_status[1]);
        switch (h_status[0]) {
        case ILUT_PIVOT: set_error("ilut: zero or non-finite pivot" + at); return cleanup(DPCG_ERR_PIVOT);
        case ILUT_CAND: set_error("ilut: more than 256 positions in a working row" + at); return cleanup(DPCG_ERR_INVALID);
        default: set_error("ilut: a row of L or U would keep more than 64 entries" + at); return cleanup(DPCG_ERR_INVALID);
        }
    }
    const unsigned grid = (unsigned)((n + 1 + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_ilut_count, dim3(grid), dim3(kBlock), 0, s, (int)n, lcnt, ucnt, cl, cu);
    if ((st = exclusive_scan_i32(cl, Lf.rowptr, n + 1, s)) < 0) return cleanup(st);
    if ((st = exclusive_scan_i32(cu, Uf.rowptr, n + 1, s)) < 0) return cleanup(st);
    int32_t lnnz = 0, unnz = 0;
    e = hipMemcpyAsync(&lnnz, Lf.rowptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&unnz, Uf.rowptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return cleanup(hip_fail(e, "ilut: row pointers", __FILE__, __LINE__));
    Lf.nnz = lnnz;
    Uf.nnz = unnz;
    if ((st = dev_alloc(&Lf.col, lnnz)) < 0 || (st = dev_alloc(&Lf.val, lnnz)) < 0 || (st = dev_alloc(&Uf.col, unnz)) < 0 ||
        (st = dev_alloc(&Uf.val, unnz)) < 0)
        return cleanup(st);
    hipLaunchKernelGGL(k_ilut_emit, dim3(grid), dim3(kBlock), 0, s, (int)n, lcnt, lcol, lval, ucnt, ucol, uval, udiag, Lf.rowptr,
                       Lf.col, Lf.val, Uf.rowptr, Uf.col, Uf.val);
    e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return cleanup(hip_fail(e, "ilut: emit", __FILE__, __LINE__));
    return cleanup(DPCG_OK);
}
