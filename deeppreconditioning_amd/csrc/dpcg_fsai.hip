// The factorised sparse approximate inverse (FSAI; Kolotilina & Yeremin 1993): the device routine behind dpcg_set_precond_fsai and
// dpcg_set_precond_fsai_pattern (contract: tests/fsai_restatement.py and the comment in include/dpcg.h).  For a symmetric pattern P
// with the diagonal, column i of the factor solves the dense SPD system A[P_i, P_i] y = e_1 on P_i = { j >= i : (j, i) in P } and
// L[P_i, i] = y / sqrt(y_1): M = L L^T ~ A^-1, only ever multiplied.  The n local systems are independent: no level schedule.
//
// Symbolic phase (once per pattern, kept in FsaiCache):
//   - the pattern of A^k: X_0 = I, X_{s+1} = pattern(X_s A); one step expands the products of every row into keys row << 32 | col,
//     sorts them (radix sort) and keeps one of each; the last step keeps columns >= row only -- the upper triangle by rows = the
//     sets P_i.  (The SpGEMM of dpcg_amg.hip sorts each row in LDS with values attached; here there are no values and the rows of
//     A^2 / A^3 outgrow its LDS rows, so the expansion is sorted as a whole.)  An explicit lower pattern is transposed instead.
//   - m_i, the columns sorted by width class (m <= 4, 8, 16, 32, 64), L's pattern = the transpose of H's with the entry map;
//   - the gather map: for every pair (p, q <= p) of P_i the entry of A that holds A[P_i[p], P_i[q]], or -1.  It is always built
//     (sum of m_i (m_i + 1) / 2 int32: 91 per column for level 2 on a 7-point grid, 364 MB at 1 M rows; the cap is 2^31 entries,
//     beyond it the call fails with DPCG_ERR_INVALID) -- the numeric phase then never searches.
// Numeric phase (every attach): batched dense Cholesky solves by width class, operation order as in tests/fsai_restatement.py.
//   - m <= 4, m <= 8 (k_fsai_reg): one column per lane, the packed triangle in registers, every loop unrolled; the map of these
//     classes is stored entry-major ([t][column]) so that a wave's loads coalesce.
//   - m <= 16, 32, 64 (k_fsai_wide): W lanes per column (4, 2, 1 columns per wave), the packed triangle in LDS (W (W + 1) / 2
//     doubles: 16.6 KB at W = 64), lane p owns row p.  Left-looking Cholesky: at step j lane p forms s = b_pj - sum_k c_pk c_jk with
//     k ascending, the pivot travels by a cross-lane read; the two substitutions are column-oriented, s_p in a register.  A wave only
//     talks to itself: wave barriers, no workgroup barrier.
//   The values land in H = L^T by rows (row i = the solve of column i) and are gathered into L through the entry map.
#include <algorithm>

#include "dpcg_host.h"
#include "dpcg_prims.h"

namespace dpcg {

// What the symbolic phase leaves on the handle (dpcg_system::fsai), keyed on level | explicit pattern.
struct FsaiCache {
    int level = -1;                       // 1 .. 3; 0: an explicit pattern
    int64_t n = 0, nnz = 0;               // entries of H = L^T (and of L)
    int32_t *pat_rp = nullptr, *pat_ci = nullptr;   // the explicit pattern as given (the key)
    int64_t pat_nnz = 0;
    int32_t *hrp = nullptr, *hci = nullptr;         // H by rows: row i lists P_i ascending
    int32_t *lrp = nullptr, *lci = nullptr;         // L by rows (columns ascending, diagonal last)
    int32_t *t_order = nullptr;                     // entry of L -> entry of H
    int32_t *order = nullptr;                       // the columns sorted by width class (stable)
    int32_t *moff = nullptr;                        // sorted position -> where its triangle starts in `map` (wide classes)
    int32_t *map = nullptr;                         // the gather map: [wide classes, column by column][m <= 4: 10 x nb][m <= 8: 36 x nb]
    int bin_ptr[6] = {0, 0, 0, 0, 0, 0};            // sorted positions of the five classes
    int64_t reg_base[2] = {0, 0};                   // where the two entry-major blocks start in `map`
    int max_m = 0;
    bool attached = false;                          // the handle's current preconditioner is this factor
    bool reused = false;                            // the last attach found the symbolic phase done
};

namespace {

constexpr int kFsaiMaxM = 64;
constexpr int kNoColumn = 0x7fffffff;

constexpr int kFsaiGrid = 65535;      // most workgroups of a setup kernel

__host__ __device__ inline int width_class(int m) { return m <= 4 ? 0 : m <= 8 ? 1 : m <= 16 ? 2 : m <= 32 ? 3 : 4; }

// ---- symbolic phase ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_identity(int64_t n, int32_t *__restrict__ rp, int32_t *__restrict__ ci) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
        rp[i] = (int32_t)i;
        if (i < n) ci[i] = (int32_t)i;
    }
}

// first row of A without a stored diagonal -> *first (atomicMin); first row whose columns do not strictly ascend -> *unsorted
// (find_entry searches A's rows by bisection: on any other row it would miss stored entries and the gather map read them as 0)
__global__ __launch_bounds__(kBlock) void k_check_rows(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, int *first,
                                                       int *unsorted) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        bool have = false, asc = true;
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            have |= ci[k] == i;
            asc &= k + 1 >= rp[i + 1] || ci[k] < ci[k + 1];
        }
        if (!have) atomicMin(first, (int)i);
        if (!asc) atomicMin(unsorted, (int)i);
    }
}

// products of row i of X A (columns >= i only when `upper`); cnt[n] = 0; *total += their number (64 bits)
__global__ __launch_bounds__(kBlock) void k_expand_count(int64_t n, const int32_t *__restrict__ xrp, const int32_t *__restrict__ xci,
                                                         const int32_t *__restrict__ arp, const int32_t *__restrict__ aci, int upper,
                                                         int32_t *__restrict__ cnt, unsigned long long *total) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    unsigned long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
        int64_t c = 0;
        if (i < n)
            for (int k = xrp[i]; k < xrp[i + 1]; ++k) {
                const int a = xci[k];
                if (!upper) {
                    c += arp[a + 1] - arp[a];
                } else {
                    for (int t = arp[a]; t < arp[a + 1]; ++t) c += aci[t] >= i ? 1 : 0;
                }
            }
        cnt[i] = (int32_t)std::min<int64_t>(c, 0x7fffffff);
        mine += (unsigned long long)c;
    }
    if (mine) atomicAdd(total, mine);
}

__global__ __launch_bounds__(kBlock) void k_expand_fill(int64_t n, const int32_t *__restrict__ xrp, const int32_t *__restrict__ xci,
                                                        const int32_t *__restrict__ arp, const int32_t *__restrict__ aci, int upper,
                                                        const int32_t *__restrict__ off, uint64_t *__restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int64_t o = off[i];
        for (int k = xrp[i]; k < xrp[i + 1]; ++k) {
            const int a = xci[k];
            for (int t = arp[a]; t < arp[a + 1]; ++t) {
                const int j = aci[t];
                if (upper && j < i) continue;
                key[o++] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)j;
            }
        }
    }
}

// head[t] = 1 where sorted key t differs from its predecessor; head[count] = 0
__global__ __launch_bounds__(kBlock) void k_heads(int64_t count, const uint64_t *__restrict__ key, int32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t <= count; t += stride)
        head[t] = t < count && (t == 0 || key[t] != key[t - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_compact(int64_t count, const uint64_t *__restrict__ key, const int32_t *__restrict__ head,
                                                    const int32_t *__restrict__ pos, uint32_t *__restrict__ row, int32_t *__restrict__ col) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < count; t += stride)
        if (head[t]) {
            row[pos[t]] = (uint32_t)(key[t] >> 32);
            col[pos[t]] = (int32_t)(uint32_t)key[t];
        }
}

// an explicit pattern: lower triangular, ascending columns, the diagonal last in every row (bit 0: not so; bit 1: no diagonal)
__global__ __launch_bounds__(kBlock) void k_check_pattern(int64_t n, int64_t nnz, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                          int *flags) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int64_t a = rp[i], b = rp[i + 1];
        if (a < 0 || b < a || b > nnz || (i == 0 && a != 0)) {
            bad |= 1;
            continue;
        }
        if (b == a || ci[b - 1] != i) bad |= 2;
        for (int64_t k = a; k < b; ++k) {
            if (ci[k] < 0 || ci[k] > i) bad |= 1;
            if (k + 1 < b && ci[k] >= ci[k + 1]) bad |= 1;
        }
    }
    if (bad) atomicOr(flags, bad);
}

// m_i, its width class as a sort key, the first column wider than the cap
__global__ __launch_bounds__(kBlock) void k_widths(int64_t n, const int32_t *__restrict__ hrp, int32_t *__restrict__ m, uint32_t *__restrict__ cls,
                                                   int *first_wide) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int mi = hrp[i + 1] - hrp[i];
        m[i] = mi;
        cls[i] = (uint32_t)width_class(mi);
        if (mi > kFsaiMaxM) atomicMin(first_wide, (int)i);
    }
}

// triangle sizes of the sorted columns (0 for the register classes, whose map is entry-major); tri[n] = 0
__global__ __launch_bounds__(kBlock) void k_tri_sizes(int64_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ m, int wide0,
                                                      int32_t *__restrict__ tri) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s <= n; s += stride) {
        int v = 0;
        if (s < n && s >= wide0) {
            const int mi = m[order[s]];
            v = mi * (mi + 1) / 2;
        }
        tri[s] = v;
    }
}

// the entry of A that holds A[r, c] (columns of a row ascending), or -1
__device__ __forceinline__ int find_entry(const int32_t *__restrict__ arp, const int32_t *__restrict__ aci, int r, int c) {
    int lo = arp[r], hi = arp[r + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (aci[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < arp[r + 1] && aci[lo] == c ? lo : -1;
}

// register classes: map[t * nb + c] for the W (W + 1) / 2 pairs t = p (p + 1) / 2 + q of the c-th column of the class (-1 beyond m)
__global__ __launch_bounds__(kBlock) void k_map_reg(int nb, int W, const int32_t *__restrict__ order, const int32_t *__restrict__ hrp,
                                                    const int32_t *__restrict__ hci, const int32_t *__restrict__ arp,
                                                    const int32_t *__restrict__ aci, int32_t *__restrict__ map) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < nb; c += stride) {
        const int i = order[c], h0 = hrp[i], m = hrp[i + 1] - h0;
        int t = 0;
        for (int p = 0; p < W; ++p)
            for (int q = 0; q <= p; ++q, ++t) map[(int64_t)t * nb + c] = p < m ? find_entry(arp, aci, hci[h0 + p], hci[h0 + q]) : -1;
    }
}

// wide classes: W threads per column, the triangle of sorted position s at map[moff[s] ..]
__global__ __launch_bounds__(kBlock) void k_map_wide(int s0, int nb, int W, const int32_t *__restrict__ order, const int32_t *__restrict__ hrp,
                                                     const int32_t *__restrict__ hci, const int32_t *__restrict__ moff,
                                                     const int32_t *__restrict__ arp, const int32_t *__restrict__ aci, int32_t *__restrict__ map) {
    const int per = kBlock / W;
    const int lane = threadIdx.x % W;
    for (int64_t c = (int64_t)blockIdx.x * per + threadIdx.x / W; c < nb; c += (int64_t)gridDim.x * per) {
        const int i = order[s0 + c], h0 = hrp[i], m = hrp[i + 1] - h0, T = m * (m + 1) / 2;
        const int64_t base = moff[s0 + c];
        for (int t = lane; t < T; t += W) {
            int p = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while ((p + 1) * (p + 2) / 2 <= t) ++p;
            while (p * (p + 1) / 2 > t) --p;
            const int q = t - p * (p + 1) / 2;
            map[base + t] = find_entry(arp, aci, hci[h0 + p], hci[h0 + q]);
        }
    }
}

// ---- numeric phase ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool good_pivot(double s) { return s > 0.0 && __builtin_isfinite(s); }

// One column per lane, m <= W (W = 4, 8): the triangle in registers.  Entries beyond m are padded with the identity, which leaves the
// leading m x m block of the Cholesky factor and the forward substitution as they are; the backward substitution skips them.
template <int W>
__global__ __launch_bounds__(kBlock) void k_fsai_reg(int nb, const int32_t *__restrict__ order, const int32_t *__restrict__ hrp,
                                                     const int32_t *__restrict__ map, const double *__restrict__ av, double *__restrict__ hv,
                                                     int *first_bad) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nb) return;
    const int i = order[c], h0 = hrp[i], m = hrp[i + 1] - h0;
    double a[W * (W + 1) / 2];
#pragma unroll
    for (int p = 0; p < W; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) {
            const int t = p * (p + 1) / 2 + q;
            const int e = map[(int64_t)t * nb + c];
            a[t] = e >= 0 ? av[e] : (p == q && p >= m) ? 1.0 : 0.0;
        }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        double d = 1.0;
#pragma unroll
        for (int p = j; p < W; ++p) {
            double s = a[p * (p + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - a[p * (p + 1) / 2 + k] * a[j * (j + 1) / 2 + k];
            if (p == j) {
                bad |= j < m && !good_pivot(s);
                d = sqrt(s);
                a[p * (p + 1) / 2 + j] = d;
            } else {
                a[p * (p + 1) / 2 + j] = s / d;
            }
        }
    }
    double s[W], y[W];
#pragma unroll
    for (int p = 0; p < W; ++p) s[p] = p == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        s[j] = s[j] / a[j * (j + 1) / 2 + j];                 // w_j
#pragma unroll
        for (int p = j + 1; p < W; ++p) s[p] = s[p] - a[p * (p + 1) / 2 + j] * s[j];
    }
#pragma unroll
    for (int j = W - 1; j >= 0; --j) {
        y[j] = s[j] / a[j * (j + 1) / 2 + j];
#pragma unroll
        for (int p = 0; p < j; ++p) s[p] = j < m ? s[p] - a[j * (j + 1) / 2 + p] * y[j] : s[p];
    }
    bad |= !good_pivot(y[0]);
    if (bad) {
        atomicMin(first_bad, i);
        return;
    }
    const double scale = sqrt(y[0]);
#pragma unroll
    for (int p = 0; p < W; ++p)
        if (p < m) hv[h0 + p] = y[p] / scale;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// W lanes per column, m <= W (W = 16, 32, 64): the packed triangle in LDS, lane p owns row p.  Every loop bound is the widest m of
// the wave, so the cross-lane reads and the wave barriers are reached by all 64 lanes.
template <int W>
__global__ __launch_bounds__(kBlock) void k_fsai_wide(int s0, int nb, const int32_t *__restrict__ order, const int32_t *__restrict__ hrp,
                                                      const int32_t *__restrict__ moff, const int32_t *__restrict__ map,
                                                      const double *__restrict__ av, double *__restrict__ hv, int *first_bad) {
    constexpr int T = W * (W + 1) / 2;
    constexpr int kPer = kBlock / W;                           // columns per workgroup
    __shared__ double tri_all[kPer * T];
    const int g = threadIdx.x / W, p = threadIdx.x % W;
    double *tri = tri_all + g * T;
    const int64_t c = (int64_t)blockIdx.x * kPer + g;
    const bool valid = c < nb;
    const int i = valid ? order[s0 + c] : 0;
    const int h0 = valid ? hrp[i] : 0;
    const int m = valid ? hrp[i + 1] - h0 : 0;
    int mmax = m;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o));
    if (valid) {
        const int64_t base = moff[s0 + c];
        for (int t = p; t < m * (m + 1) / 2; t += W) {
            const int e = map[base + t];
            tri[t] = e >= 0 ? av[e] : 0.0;
        }
    }
    wave_sync();
    const int rowp = p * (p + 1) / 2;
    bool bad = false;
    for (int j = 0; j < mmax; ++j) {
        const bool act = p >= j && p < m;                     // (p < m and p >= j: j < m)
        const int rowj = j * (j + 1) / 2;
        double s = act ? tri[rowp + j] : 1.0;
        for (int k = 0; k < j; ++k)
            if (act) s = s - tri[rowp + k] * tri[rowj + k];
        const double piv = __shfl(s, j, W);
        if (act && p == j) bad = !good_pivot(s);
        const double d = sqrt(piv);
        if (act) tri[rowp + j] = p == j ? d : s / d;
        wave_sync();
    }
    // C w = e_1
    double s = p == 0 ? 1.0 : 0.0;
    for (int j = 0; j < mmax; ++j) {
        const bool in = j < m;
        const double cjj = in ? tri[j * (j + 1) / 2 + j] : 1.0;
        const double wj = __shfl(s, j, W) / cjj;
        if (p == j) s = wj;
        if (in && p > j && p < m) s = s - tri[rowp + j] * wj;
    }
    // C^T y = w
    for (int j = mmax - 1; j >= 0; --j) {
        const bool in = j < m;
        const int rowj = j * (j + 1) / 2;
        const double cjj = in ? tri[rowj + j] : 1.0;
        const double yj = __shfl(s, j, W) / cjj;
        if (p == j) s = yj;
        if (in && p < j) s = s - tri[rowj + p] * yj;
    }
    const double y0 = __shfl(s, 0, W);
    if (valid && p == 0 && !good_pivot(y0)) bad = true;
    if (bad) atomicMin(first_bad, i);
    if (valid && p < m) hv[h0 + p] = s / sqrt(y0);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// One step X -> pattern(X A) (columns >= row only when `upper`): owned (rp, ci) and the entry count
int power_step(int64_t n, const int32_t *xrp, const int32_t *xci, const CsrDev &A, bool upper, DevBuf<int32_t> &out_rp, DevBuf<int32_t> &out_ci,
               int64_t *out_nnz, hipStream_t s) {
    DevBuf<int32_t> cnt, off, head, pos, vin, vout;
    DevBuf<unsigned long long> total;
    DevBuf<uint64_t> key, key_sorted;
    DevBuf<uint32_t> rows;
    DPCG_TRY(cnt.alloc(n + 1));
    DPCG_TRY(off.alloc(n + 1));
    DPCG_TRY(total.alloc(1));
    DPCG_HIP(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_expand_count, dim3(grid_blocks(n + 1, kFsaiGrid)), dim3(kBlock), 0, s, n, xrp, xci, A.rowptr, A.col, upper ? 1 : 0, cnt.p, total.p);
    unsigned long long h_total = 0;
    DPCG_TRY(fetch(&h_total, total.p, 1, s));
    if (h_total >= 0x7fffffffull) return invalid("dpcg_set_precond_fsai: the pattern of A^k expands to more than 2^31 products");
    const int64_t count = (int64_t)h_total;
    DPCG_TRY(exclusive_scan_i32(cnt.p, off.p, n + 1, s));
    DPCG_TRY(key.alloc(count));
    DPCG_TRY(key_sorted.alloc(count));
    DPCG_TRY(vin.alloc(count));
    DPCG_TRY(vout.alloc(count));
    hipLaunchKernelGGL(k_expand_fill, dim3(grid_blocks(n, kFsaiGrid)), dim3(kBlock), 0, s, n, xrp, xci, A.rowptr, A.col, upper ? 1 : 0, off.p, key.p);
    launch_iota(count, vin.p, s);
    DPCG_TRY(sort_pairs_u64_i32(key.p, key_sorted.p, vin.p, vout.p, count, 32 + bits_for((uint64_t)(n - 1)), s));
    DPCG_TRY(head.alloc(count + 1));
    DPCG_TRY(pos.alloc(count + 1));
    hipLaunchKernelGGL(k_heads, dim3(grid_blocks(count + 1, kFsaiGrid)), dim3(kBlock), 0, s, count, key_sorted.p, head.p);
    DPCG_TRY(exclusive_scan_i32(head.p, pos.p, count + 1, s));
    int32_t uniq = 0;
    DPCG_TRY(fetch(&uniq, pos.p + count, 1, s));
    DPCG_TRY(rows.alloc(uniq));
    DPCG_TRY(out_rp.alloc(n + 1));
    DPCG_TRY(out_ci.alloc(uniq));
    hipLaunchKernelGGL(k_compact, dim3(grid_blocks(count, kFsaiGrid)), dim3(kBlock), 0, s, count, key_sorted.p, head.p, pos.p, rows.p, out_ci.p);
    launch_group_offsets(uniq, rows.p, (int)n, out_rp.p, s);
    DPCG_HIP(hipStreamSynchronize(s));
    DPCG_CHECK_LAUNCH();
    *out_nnz = uniq;
    return DPCG_OK;
}

void free_cache_arrays(FsaiCache &c) {
    dev_free(c.pat_rp); dev_free(c.pat_ci); dev_free(c.hrp); dev_free(c.hci); dev_free(c.lrp); dev_free(c.lci);
    dev_free(c.t_order); dev_free(c.order); dev_free(c.moff); dev_free(c.map);
}

// The symbolic phase into `c` (c.level, and c.pat_* for an explicit pattern, are set; c.hrp / c.hci hold the sets P_i)
int symbolic_rest(FsaiCache &c, const CsrDev &A, hipStream_t s) {
    const int64_t n = c.n, nnz = c.nnz;
    // widths, the cap, the classes
    DevBuf<int32_t> m, iota, tri;
    DevBuf<uint32_t> cls, cls_sorted;
    DevBuf<int> first;
    DevBuf<int32_t> binp;
    DPCG_TRY(m.alloc(n));
    DPCG_TRY(cls.alloc(n));
    DPCG_TRY(cls_sorted.alloc(n));
    DPCG_TRY(iota.alloc(n));
    DPCG_TRY(first.alloc(1));
    DPCG_TRY(binp.alloc(6));
    const int none = kNoColumn;
    DPCG_HIP(hipMemcpyAsync(first.p, &none, sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_widths, dim3(grid_blocks(n, kFsaiGrid)), dim3(kBlock), 0, s, n, c.hrp, m.p, cls.p, first.p);
    int h_first = kNoColumn;
    DPCG_TRY(fetch(&h_first, first.p, 1, s));
    if (h_first != kNoColumn) {
        int32_t wm = 0;
        DPCG_TRY(fetch(&wm, m.p + h_first, 1, s));
        set_error("fsai: column " + std::to_string(h_first) + " has m = " + std::to_string(wm) + " > " + std::to_string(kFsaiMaxM) +
                  " entries in its local system");
        return DPCG_ERR_INVALID;
    }
    DevBuf<int32_t> mmax;
    DPCG_TRY(mmax.alloc(1));
    DPCG_TRY(reduce_max_i32(m.p, mmax.p, n, s));
    int32_t h_mmax = 0;
    DPCG_TRY(fetch(&h_mmax, mmax.p, 1, s));
    c.max_m = h_mmax;
    DPCG_TRY(dev_alloc(&c.order, n));
    launch_iota(n, iota.p, s);
    DPCG_TRY(sort_pairs_u32_i32(cls.p, cls_sorted.p, iota.p, c.order, n, 3, s));
    launch_group_offsets(n, cls_sorted.p, 5, binp.p, s);
    int32_t h_bin[6];
    DPCG_TRY(fetch(h_bin, binp.p, 6, s));
    for (int b = 0; b < 6; ++b) c.bin_ptr[b] = h_bin[b];
    // the gather map
    const int64_t wide_bound = (int64_t)(n - c.bin_ptr[2]) * (kFsaiMaxM * (kFsaiMaxM + 1) / 2);
    DPCG_TRY(tri.alloc(n + 1));
    DPCG_TRY(dev_alloc(&c.moff, n + 1));
    hipLaunchKernelGGL(k_tri_sizes, dim3(grid_blocks(n + 1, kFsaiGrid)), dim3(kBlock), 0, s, n, c.order, m.p, c.bin_ptr[2], tri.p);
    if (wide_bound >= 0x7fffffffll) {                        // (only then can the int32 scan wrap: sum the sizes in 64 bits first)
        std::vector<int32_t> h_tri((size_t)n + 1);
        DPCG_TRY(fetch(h_tri.data(), tri.p, n + 1, s));
        int64_t sum = 0;
        for (int32_t v : h_tri) sum += v;
        if (sum >= 0x7fffffffll) return invalid("fsai: the gather map of this pattern needs more than 2^31 entries");
    }
    DPCG_TRY(exclusive_scan_i32(tri.p, c.moff, n + 1, s));
    int32_t wide_len = 0;
    DPCG_TRY(fetch(&wide_len, c.moff + n, 1, s));
    const int64_t nb0 = c.bin_ptr[1] - c.bin_ptr[0], nb1 = c.bin_ptr[2] - c.bin_ptr[1];
    c.reg_base[0] = wide_len;
    c.reg_base[1] = c.reg_base[0] + 10 * nb0;
    const int64_t map_len = c.reg_base[1] + 36 * nb1;
    DPCG_TRY(dev_alloc(&c.map, map_len));
    if (nb0 > 0)
        hipLaunchKernelGGL(k_map_reg, dim3(grid_blocks(nb0, kFsaiGrid)), dim3(kBlock), 0, s, (int)nb0, 4, c.order + c.bin_ptr[0], c.hrp, c.hci, A.rowptr, A.col,
                           c.map + c.reg_base[0]);
    if (nb1 > 0)
        hipLaunchKernelGGL(k_map_reg, dim3(grid_blocks(nb1, kFsaiGrid)), dim3(kBlock), 0, s, (int)nb1, 8, c.order + c.bin_ptr[1], c.hrp, c.hci, A.rowptr, A.col,
                           c.map + c.reg_base[1]);
    for (int b = 2; b < 5; ++b) {
        const int nb = c.bin_ptr[b + 1] - c.bin_ptr[b], W = 16 << (b - 2);
        if (nb == 0) continue;
        const int per = kBlock / W;
        const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)nb + per - 1) / per, 1 << 20);
        hipLaunchKernelGGL(k_map_wide, dim3(grid), dim3(kBlock), 0, s, c.bin_ptr[b], nb, W, c.order, c.hrp, c.hci, c.moff, A.rowptr, A.col, c.map);
    }
    // L's pattern: the transpose of H's
    DPCG_TRY(dev_alloc(&c.lrp, n + 1));
    DPCG_TRY(dev_alloc(&c.lci, nnz));
    DPCG_TRY(dev_alloc(&c.t_order, nnz));
    DPCG_TRY(transpose_csr(n, n, nnz, c.hrp, c.hci, nullptr, c.lrp, c.lci, nullptr, c.t_order, s));
    DPCG_HIP(hipStreamSynchronize(s));
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

int symbolic(FsaiCache &c, const CsrDev &A, hipStream_t s) {
    const int64_t n = A.n;
    c.n = n;
    {
        DevBuf<int> first;
        DPCG_TRY(first.alloc(2));
        const int none[2] = {kNoColumn, kNoColumn};
        DPCG_HIP(hipMemcpyAsync(first.p, none, sizeof(none), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_check_rows, dim3(grid_blocks(n, kFsaiGrid)), dim3(kBlock), 0, s, n, A.rowptr, A.col, first.p, first.p + 1);
        int h_first[2] = {kNoColumn, kNoColumn};
        DPCG_TRY(fetch(h_first, first.p, 2, s));
        if (h_first[1] != kNoColumn) {
            set_error("fsai: the matrix must have strictly ascending columns in every row (row " + std::to_string(h_first[1]) + " has not)");
            return DPCG_ERR_INVALID;
        }
        if (c.level > 0 && h_first[0] != kNoColumn) {
            set_error("fsai: structurally missing diagonal at column " + std::to_string(h_first[0]));
            return DPCG_ERR_INVALID;
        }
    }
    if (c.level > 0) {
        DevBuf<int32_t> xrp, xci;
        DPCG_TRY(xrp.alloc(n + 1));
        DPCG_TRY(xci.alloc(n));
        hipLaunchKernelGGL(k_identity, dim3(grid_blocks(n + 1, kFsaiGrid)), dim3(kBlock), 0, s, n, xrp.p, xci.p);
        int64_t xnnz = n;
        for (int step = 1; step <= c.level; ++step) {
            DevBuf<int32_t> yrp, yci;
            DPCG_TRY(power_step(n, xrp.p, xci.p, A, step == c.level, yrp, yci, &xnnz, s));
            std::swap(xrp.p, yrp.p);
            std::swap(xci.p, yci.p);
        }
        c.hrp = xrp.release();
        c.hci = xci.release();
        c.nnz = xnnz;
    } else {
        c.nnz = c.pat_nnz;
        DevBuf<int32_t> order;
        DPCG_TRY(order.alloc(c.nnz));
        DPCG_TRY(dev_alloc(&c.hrp, n + 1));
        DPCG_TRY(dev_alloc(&c.hci, c.nnz));
        DPCG_TRY(transpose_csr(n, n, c.nnz, c.pat_rp, c.pat_ci, nullptr, c.hrp, c.hci, nullptr, order.p, s));
        DPCG_HIP(hipStreamSynchronize(s));
        DPCG_CHECK_LAUNCH();
    }
    return symbolic_rest(c, A, s);
}

// The values of H for the handle's current matrix values, gathered into Lf (owned; the pattern copied from the cache)
int numeric(const FsaiCache &c, const CsrDev &A, CsrDev &Lf, hipStream_t s) {
    const int64_t n = c.n, nnz = c.nnz;
    DevBuf<double> hv;
    DevBuf<int> bad;
    DPCG_TRY(hv.alloc(nnz));
    DPCG_TRY(bad.alloc(1));
    const int none = kNoColumn;
    DPCG_HIP(hipMemcpyAsync(bad.p, &none, sizeof(int), hipMemcpyHostToDevice, s));
    const int nb0 = c.bin_ptr[1] - c.bin_ptr[0], nb1 = c.bin_ptr[2] - c.bin_ptr[1];
    if (nb0 > 0)
        hipLaunchKernelGGL(k_fsai_reg<4>, dim3((nb0 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, nb0, c.order + c.bin_ptr[0], c.hrp,
                           c.map + c.reg_base[0], A.val, hv.p, bad.p);
    if (nb1 > 0)
        hipLaunchKernelGGL(k_fsai_reg<8>, dim3((nb1 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, nb1, c.order + c.bin_ptr[1], c.hrp,
                           c.map + c.reg_base[1], A.val, hv.p, bad.p);
    const int nb2 = c.bin_ptr[3] - c.bin_ptr[2], nb3 = c.bin_ptr[4] - c.bin_ptr[3], nb4 = c.bin_ptr[5] - c.bin_ptr[4];
    if (nb2 > 0)
        hipLaunchKernelGGL(k_fsai_wide<16>, dim3((nb2 + kBlock / 16 - 1) / (kBlock / 16)), dim3(kBlock), 0, s, c.bin_ptr[2], nb2, c.order, c.hrp, c.moff, c.map, A.val,
                           hv.p, bad.p);
    if (nb3 > 0)
        hipLaunchKernelGGL(k_fsai_wide<32>, dim3((nb3 + kBlock / 32 - 1) / (kBlock / 32)), dim3(kBlock), 0, s, c.bin_ptr[3], nb3, c.order, c.hrp, c.moff, c.map, A.val,
                           hv.p, bad.p);
    if (nb4 > 0)
        hipLaunchKernelGGL(k_fsai_wide<64>, dim3((nb4 + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, c.bin_ptr[4], nb4, c.order, c.hrp, c.moff, c.map, A.val,
                           hv.p, bad.p);
    int h_bad = kNoColumn;
    DPCG_HIP(hipGetLastError());
    DPCG_TRY(fetch(&h_bad, bad.p, 1, s));
    if (h_bad != kNoColumn) {
        set_error("fsai: non-positive or non-finite pivot in the local system of column " + std::to_string(h_bad));
        return DPCG_ERR_PIVOT;
    }
    Lf = CsrDev();
    Lf.n = n;
    Lf.nnz = nnz;
    Lf.owned = true;
    int st = DPCG_OK;
    if ((st = dev_alloc(&Lf.rowptr, n + 1)) < 0 || (st = dev_alloc(&Lf.col, nnz)) < 0 || (st = dev_alloc(&Lf.val, nnz)) < 0) {
        free_csr(Lf);
        return st;
    }
    hipError_t e = hipMemcpyAsync(Lf.rowptr, c.lrp, (size_t)(n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(Lf.col, c.lci, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) {
        launch_gather_f64(nnz, c.t_order, hv.p, Lf.val, s);
        e = hipStreamSynchronize(s);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        free_csr(Lf);
        return hip_fail(e, "fsai: values", __FILE__, __LINE__);
    }
    return DPCG_OK;
}

}  // namespace

}  // namespace dpcg

void free_fsai(FsaiCache *&c) {
    if (!c) return;
    free_cache_arrays(*c);
    delete c;
    c = nullptr;
}

void fsai_detach(FsaiCache *c) {
    if (c) c->attached = false;
}

void fsai_mark_attached(FsaiCache *c) {
    if (c) c->attached = true;
}

// The FSAI factor of the handle's matrix in the caller's numbering into Lf (owned: lower, columns ascending, diagonal last).
// level 1 .. 3, or level 0 with an explicit lower pattern (pat_rp / pat_ci: device arrays this call takes over, also when it fails).
// The handle's cache is replaced only when the factor of another key succeeded; Lf stays empty on failure.
int fsai_factor(dpcg_system *h, int level, int64_t pat_nnz, int32_t *pat_rp, int32_t *pat_ci, CsrDev &Lf, hipStream_t s) {
    const CsrDev &A = h->perm ? h->A_user : h->A;
    PhaseTimer pt(s);
    FsaiCache *c = h->fsai;
    bool same = c && c->level == level && c->n == A.n;
    if (same && level == 0) {
        same = c->pat_nnz == pat_nnz;
        if (same) {
            int *differ = nullptr;
            int st = dev_alloc(&differ, 1);
            int h_differ = 0;
            hipError_t e = hipSuccess;
            if (st >= 0) {
                e = hipMemsetAsync(differ, 0, sizeof(int), s);
                launch_same_i32(A.n + 1, c->pat_rp, pat_rp, differ, s);
                launch_same_i32(pat_nnz, c->pat_ci, pat_ci, differ, s);
                if (e == hipSuccess) e = hipMemcpyAsync(&h_differ, differ, sizeof(int), hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            }
            dev_free(differ);
            if (st < 0 || e != hipSuccess) {
                dev_free(pat_rp);
                dev_free(pat_ci);
                return st < 0 ? st : hip_fail(e, "fsai: pattern compare", __FILE__, __LINE__);
            }
            same = h_differ == 0;
        }
    }
    if (same) {
        dev_free(pat_rp);
        dev_free(pat_ci);
        c->reused = true;
    } else {
        FsaiCache *fresh = new FsaiCache();
        fresh->level = level;
        fresh->pat_rp = pat_rp;
        fresh->pat_ci = pat_ci;
        fresh->pat_nnz = pat_nnz;
        const int st = symbolic(*fresh, A, s);
        if (st < 0) {
            free_fsai(fresh);
            return st;
        }
        c = fresh;
        pt.mark("fsai: symbolic");
    }
    const int st = numeric(*c, A, Lf, s);
    pt.mark("fsai: numeric");
    if (c != h->fsai) {                  // (a fresh cache takes the handle's place only with a factor: the one attached stays described)
        if (st < 0) {
            free_fsai(c);
        } else {
            free_fsai(h->fsai);
            h->fsai = c;
        }
    }
    return st;
}

// An explicit pattern as given (host or device arrays) onto the device, checked: lower triangular, ascending columns, the diagonal
int fsai_upload_pattern(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, int memspace, int32_t **rp_out, int32_t **ci_out,
                        hipStream_t s) {
    *rp_out = *ci_out = nullptr;
    int32_t *rp = nullptr, *ci = nullptr;
    int *flags = nullptr;
    auto done = [&](int st) {
        dev_free(flags);
        if (st < 0) { dev_free(rp); dev_free(ci); }
        return st;
    };
    int st = DPCG_OK;
    if ((st = dev_alloc(&rp, n + 1)) < 0 || (st = dev_alloc(&ci, nnz)) < 0 || (st = dev_alloc(&flags, 1)) < 0) return done(st);
    const hipMemcpyKind kind = memspace == DPCG_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    hipError_t e = hipMemcpyAsync(rp, rowptr, (size_t)(n + 1) * sizeof(int32_t), kind, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ci, col, (size_t)nnz * sizeof(int32_t), kind, s);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, sizeof(int), s);
    int32_t h_last = 0;
    int h_flags = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_last, rp + n, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return done(hip_fail(e, "fsai: pattern upload", __FILE__, __LINE__));
    if (h_last != nnz) return done(invalid("dpcg_set_precond_fsai_pattern: rowptr[n] != nnz"));
    hipLaunchKernelGGL(k_check_pattern, dim3(grid_blocks(n, kFsaiGrid)), dim3(kBlock), 0, s, n, nnz, rp, ci, flags);
    e = hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return done(hip_fail(e, "fsai: pattern check", __FILE__, __LINE__));
    if (h_flags & 1) return done(invalid("dpcg_set_precond_fsai_pattern: the pattern must be lower triangular with ascending columns"));
    if (h_flags & 2) return done(invalid("dpcg_set_precond_fsai_pattern: the pattern must contain the diagonal (last in every row)"));
    *rp_out = rp;
    *ci_out = ci;
    return done(DPCG_OK);
}

extern "C" int dpcg_get_fsai_info(dpcg_handle_t h, int32_t out[8]) {
    if (!h || !out) return invalid("dpcg_get_fsai_info: NULL handle or output");
    const FsaiCache *c = h->fsai;
    if (!c || !c->attached || h->precond != DPCG_PRECOND_LLT_MULTIPLY) {
        set_error("dpcg_get_fsai_info: the attached preconditioner is not an FSAI factor");
        return DPCG_ERR_STATE;
    }
    out[0] = c->level;
    out[1] = c->max_m;
    for (int b = 0; b < 5; ++b) out[2 + b] = c->bin_ptr[b + 1] - c->bin_ptr[b];
    out[7] = c->reused ? 1 : 0;
    return DPCG_OK;
}
