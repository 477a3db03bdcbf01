// Smoothed-aggregation algebraic multigrid (DPCG_PRECOND_AMG, include/dpcg.h): the hierarchy is built on the device and applied
// as a V(nu, nu) cycle with damped-Jacobi smoothing inside the multi-launch PCG loop (graph capture included).  The reference's
// harness names this technique `algebraic_multigrid` (pyamg's smoothed_aggregation_solver(A).aspreconditioner(cycle="V")).
//
// Setup of level l (A_l, n_l rows; level 0 = the handle's matrix; rules that look at a row index use the CALLER's index):
//   strength   j strong for i when j != i, a_ij != 0 and |a_ij| >= theta sqrt(|a_ii a_jj|)  (k_amg_diag, k_amg_strength)
//   MIS(2)     tuples (state, splitmix64(seed, caller index), caller index), OUT < UNDECIDED < IN; a round takes the tuple
//              maximum over the closed strong neighbourhood twice (k_mis_max, reading the previous round's states only) and
//              then decides (k_mis_update): own tuple -> IN, an IN maximum -> OUT.  Rounds until nobody is undecided.
//   aggregates roots numbered by ascending caller index (flag by caller index + scan); neighbours of a root join it
//              (k_agg_near: the root is unique); the rest join their step-1-assigned strong neighbour of largest |a_ij|,
//              ties to the smaller caller index (k_agg_far)
//   T          one entry per row, 1/sqrt(|aggregate|)
//   P          (I - omega D^-1 A) T, omega = (4/3) / rho, rho = theta_max + err_max of a 30-step Lanczos estimate of the
//              spectrum of D^-1 A (dpcg_spectrum on a handle that borrows A_l): the product A T by the row-wise SpGEMM with
//              the (I - omega D^-1) epilogue fused
//   A_{l+1}    P^T (A P): two row-wise SpGEMMs (k_spgemm), P^T by a stable sort of P's entries by column
// Stop at max_coarse rows, at max_levels, or when coarsening stalls (n_c > 0.9 n).  The coarsest level is inverted densely on
// the host (Cholesky) and applied by a GEMV.
//
// SpGEMM (k_spgemm): one wave per output row.  The row's products are expanded in a fixed order (entries of X's row, then of the
// Y row each selects), keyed (column << 32 | product index), bitonic-sorted in LDS (or, for rows of more than kSgCap products, in
// a global scratch segment of their own), and compressed: the first product of every column sums the run after it in product
// order.  A symbolic pass writes the row lengths, a scan gives the row pointers, the numeric pass writes sorted columns.  No
// float atomics: two setups give the same bits.
//
// Apply (launch_amg_apply), per level: k_amg_row<PRE> (x = omega D^-1 b and r = b - A x in one pass), nu - 1 k_amg_row<SWEEP>,
// k_amg_row<PLAIN> (b_{l+1} = P^T r); k_amg_gemv on the coarsest level; then k_amg_row<ACC> (x += P x_{l+1}) and nu
// k_amg_row<POST> (x += omega D^-1 (b - A x)) -- on level 0 the last one writes z and the partials of <r, z> for PCG.
//
// Other smoothers (dpcg_set_precond_amg_smoothed); the hierarchy is the same, only the smoothing steps of a level change:
//   Gauss-Seidel  rows colour by colour (multicolor_order's perm) and the colour offsets.  A pass (k_amg_gs) updates one colour in
//                 place, x_i += dinv_i (b_i - sum a_ij x_j); a symmetric sweep is the passes 0 .. m-1, m-2 .. 0.  Pre-smoothing's first
//                 pass starts from x = 0 (it writes every row).  Levels of at most gs_block_rows() rows run all their sweeps in one
//                 workgroup (k_amg_gs_block: a block barrier between colours).  k_amg_row<RES> forms b - A x before the restriction.
//                 The last pass covers one colour, so level 0 emits no <r, z> partials and PCG sums <r, z> itself.
//   Chebyshev     (x, r = b - A x) is carried from step to step: k_amg_cheb<STEP> gathers the new x_j = x_j + d'_j,
//                 d'_j = c1 d_j + c2 (dinv_j r_j), on the fly and writes x', d' and r' = b - A x' (first step of an application:
//                 d'_j = c2 (dinv_j r_j)); pre-smoothing starts from x = 0, r = b; post-smoothing forms r with k_amg_row<RES> after the
//                 correction; the last step of a level needs no r' (k_amg_cheb<LAST>, on level 0 with the <r, z> partials).
//
// fp32 cycle (dpcg_set_precond_amg_precision with DPCG_AMG_FP32; Jacobi and Chebyshev): the hierarchy is the fp64 one; after the setup
// the values of A_l, P_l, P_l^T and dinv_l of every smoothed level are stored a second time, rounded to fp32 (k_amg_to_f32), and
// every work vector of the cycle is fp32.  The kernels are the same templates with other storage types: operands are converted
// on load, every product and sum is fp64, and whatever the fp64 cycle stores to a work vector is rounded to fp32 where it is
// computed -- also when a row gathers it on the fly (PRE's and SWEEP's y_j, Chebyshev's d'_j and x_j + d'_j).  Level 0 reads
// PCG's r and writes z in fp64 (not rounded); the dense coarse inverse stays fp64 (fp32 in, fp32 out).  Same launches as fp64.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_prims.h"

namespace dpcg {

struct AmgLevel {
    CsrDev A;                         // level 0: a view of the handle's matrix (not owned); coarser levels: owned
    double *dinv = nullptr;           // 1 / a_ii
    uint8_t *strong = nullptr;        // per entry of A: strong connection
    int8_t *roots = nullptr;          // MIS(2) result (1 = root)
    int32_t *agg = nullptr;           // aggregate of each row (this level's numbering)
    CsrDev P, Pt, AP;                 // owned; empty on the coarsest level
    int32_t *pt_order = nullptr;      // entry of P^T -> entry of P (the stable sort by column)
    int64_t nc = 0;                   // rows of the next level
    double rho = 0.0, omega = 0.0;
    int tpr_a = 2, tpr_p = 2, tpr_pt = 2;
    double *b = nullptr, *xa = nullptr, *xb = nullptr, *ra = nullptr, *rb = nullptr;   // work vectors (b: levels >= 1)
    int smoother = DPCG_AMG_JACOBI;   // what this level smooths with (a Gauss-Seidel level that could not be coloured: Jacobi)
    int32_t *gs_rows = nullptr;       // Gauss-Seidel: the rows colour by colour (n)
    int32_t *gs_off_dev = nullptr;    // ... where each colour begins in gs_rows (m + 1), for the one-workgroup sweep
    std::vector<int32_t> gs_off;      // ... the same on the host
    bool gs_block = false;            // ... the whole sweep in one workgroup
    double cheb_lo = 0.0, cheb_hi = 0.0;
    std::vector<double> cheb_c1, cheb_c2;   // Chebyshev: the coefficients of each step (c1[0] unused)
    double *da = nullptr, *db = nullptr;    // Chebyshev: the direction d, double-buffered
    // fp32 cycle: the values of A, P, P^T and dinv rounded to fp32 (patterns shared with the fp64 arrays) and the work vectors
    float *a32 = nullptr, *p32 = nullptr, *pt32 = nullptr, *dinv32 = nullptr;
    float *b32 = nullptr, *xa32 = nullptr, *xb32 = nullptr, *ra32 = nullptr, *rb32 = nullptr, *da32 = nullptr, *db32 = nullptr;
};

struct AmgState {
    double theta = 0.0;
    int max_levels = 10, max_coarse = 500, sweeps = 1;
    uint64_t seed = 0;
    int smoother = DPCG_AMG_JACOBI, degree = 2;
    double eig_ratio = 30.0;
    int precision = DPCG_AMG_FP64;    // what the cycle stores (the hierarchy is fp64 either way)
    std::vector<AmgLevel> lv;         // lv.back(): the coarsest level (dense solve)
    double *cinv = nullptr;           // dense inverse of the coarsest matrix, row-major
    int64_t nco = 0;
    int reused_levels = 0;            // levels whose structures a re-attach took over from the parked hierarchy
};

namespace {

constexpr int kSgCap = 1024;          // products of a row sorted in LDS (16 KiB per one-wave workgroup)
constexpr int kApplyMaxGrid = kMaxSpmvGrid;
constexpr int kRhoSteps = 30;         // Lanczos steps of the spectral-radius estimate
constexpr int kGsBlockThreads = 1024; // the one-workgroup Gauss-Seidel sweep

// Gauss-Seidel levels of at most this many rows sweep in one workgroup (DPCG_AMG_GS_BLOCK_ROWS overrides; DESIGN.md has the measurement)
int gs_block_rows() {
    static const int v = [] { const char *e = getenv("DPCG_AMG_GS_BLOCK_ROWS"); return e ? atoi(e) : 4096; }();
    return v;
}

enum MisState : int8_t { MIS_OUT = 0, MIS_UND = 1, MIS_IN = 2 };
constexpr int kAmgGrid = 65536;       // most workgroups of a setup or cycle kernel that strides over its items

__device__ __forceinline__ uint64_t amg_hash(uint64_t seed, uint64_t i) {   // splitmix64 finaliser of a counter (as k_lz_start)
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + (i + 1) * 0xBF58476D1CE4E5B9ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}


// ---- setup kernels ---------------------------------------------------------------------------------------------
// dinv[i] = 1 / a_ii; *bad |= 1 when a diagonal is missing, zero, negative or not finite
__global__ __launch_bounds__(kBlock) void k_amg_diag(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                     const double *__restrict__ v, double *__restrict__ dinv,
                                                     double *__restrict__ diag, int *bad) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double d = 0.0;
        for (int k = rp[i]; k < rp[i + 1]; ++k)
            if (ci[k] == i) d = v[k];
        if (!(d > 0.0) || !isfinite(d)) {
            atomicOr(bad, 1);
            dinv[i] = 0.0;
        } else {
            dinv[i] = 1.0 / d;
        }
        if (diag) diag[i] = d;
    }
}

__global__ __launch_bounds__(kBlock) void k_amg_strength(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                         const double *__restrict__ v, const double *__restrict__ diag, double theta,
                                                         uint8_t *__restrict__ strong) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            const int j = ci[k];
            const double dij = diag[i] * diag[j];
            strong[k] = (j != i && v[k] != 0.0 && fabs(v[k]) >= theta * sqrt(fabs(dij))) ? 1 : 0;
        }
}

__global__ __launch_bounds__(kBlock) void k_mis_init(int64_t n, uint64_t seed, const int32_t *__restrict__ perm,
                                                     int8_t *__restrict__ st, uint64_t *__restrict__ hsh, int32_t *__restrict__ cid) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int32_t c = perm ? perm[i] : (int32_t)i;
        st[i] = MIS_UND;
        cid[i] = c;
        hsh[i] = amg_hash(seed, (uint64_t)c);
    }
}

__device__ __forceinline__ bool tuple_gt(int a, int b, const int8_t *st, const uint64_t *hsh, const int32_t *cid) {
    if (st[a] != st[b]) return st[a] > st[b];
    if (hsh[a] != hsh[b]) return hsh[a] > hsh[b];
    return cid[a] > cid[b];
}

// out[i] = the node of largest tuple among {in[i]} and {in[j] : j strong neighbour of i} (in = null: the nodes themselves)
__global__ __launch_bounds__(kBlock) void k_mis_max(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const uint8_t *__restrict__ strong, const int8_t *__restrict__ st,
                                                    const uint64_t *__restrict__ hsh, const int32_t *__restrict__ cid,
                                                    const int32_t *__restrict__ in, int32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int best = in ? in[i] : (int)i;
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            const int j = ci[k];
            if (j == i || (strong && !strong[k])) continue;
            const int c = in ? in[j] : j;
            if (tuple_gt(c, best, st, hsh, cid)) best = c;
        }
        out[i] = best;
    }
}

__global__ __launch_bounds__(kBlock) void k_mis_update(int64_t n, const int8_t *__restrict__ st, const int32_t *__restrict__ m2,
                                                       int8_t *__restrict__ st_new, int *undecided) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int left = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int8_t s = st[i];
        if (s == MIS_UND) {
            const int J = m2[i];
            if (J == i) s = MIS_IN;
            else if (st[J] == MIS_IN) s = MIS_OUT;
            else left = 1;
        }
        st_new[i] = s;
    }
    if (left) atomicAdd(undecided, 1);
}

__global__ __launch_bounds__(kBlock) void k_root_flags(int64_t n, const int8_t *__restrict__ st, const int32_t *__restrict__ cid,
                                                       int8_t *__restrict__ roots, int32_t *__restrict__ flag_by_cid) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        roots[i] = st[i] == MIS_IN ? 1 : 0;
        flag_by_cid[cid[i]] = st[i] == MIS_IN ? 1 : 0;
    }
}

// roots: their number; neighbours of a root: the root's (unique: roots are >= 3 hops apart); others -1
__global__ __launch_bounds__(kBlock) void k_agg_near(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                     const uint8_t *__restrict__ strong, const int8_t *__restrict__ roots,
                                                     const int32_t *__restrict__ cid, const int32_t *__restrict__ rank_by_cid,
                                                     int32_t *__restrict__ agg1) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int a = -1;
        if (roots[i]) {
            a = rank_by_cid[cid[i]];
        } else {
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int j = ci[k];
                if (j == i || (strong && !strong[k])) continue;
                if (roots[j]) { a = rank_by_cid[cid[j]]; break; }
            }
        }
        agg1[i] = a;
    }
}

// the rest: the aggregate of the step-1-assigned strong neighbour of largest |a_ij| (ties: smaller caller index)
__global__ __launch_bounds__(kBlock) void k_agg_far(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const double *__restrict__ v, const uint8_t *__restrict__ strong,
                                                    const int32_t *__restrict__ cid, const int32_t *__restrict__ agg1,
                                                    int32_t *__restrict__ agg, int *bad) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int a = agg1[i];
        if (a < 0) {
            double best = -1.0;
            int bc = 0x7fffffff;
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int j = ci[k];
                if (j == i || (strong && !strong[k]) || agg1[j] < 0) continue;
                const double w = fabs(v[k]);
                if (w > best || (w == best && cid[j] < bc)) { best = w; bc = cid[j]; a = agg1[j]; }
            }
            if (a < 0) atomicOr(bad, 2);
        }
        agg[i] = a < 0 ? 0 : a;
    }
}

__global__ __launch_bounds__(kBlock) void k_agg_size(int64_t n, const int32_t *__restrict__ agg, int32_t *__restrict__ size) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) atomicAdd(&size[agg[i]], 1);   // (integers)
}

// T as CSR: one entry per row
__global__ __launch_bounds__(kBlock) void k_tentative(int64_t n, const int32_t *__restrict__ agg, const int32_t *__restrict__ size,
                                                      int32_t *__restrict__ rp, int32_t *__restrict__ ci, double *__restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
        rp[i] = (int32_t)i;
        if (i < n) {
            ci[i] = agg[i];
            v[i] = 1.0 / sqrt((double)size[agg[i]]);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_diff_i32(int64_t n, const int32_t *__restrict__ a, const int32_t *__restrict__ b, int *diff) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        if (a[i] != b[i]) atomicOr(diff, 1);
}

// ---- row-wise SpGEMM C = X Y ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sg_products(int64_t m, const int32_t *__restrict__ xrp, const int32_t *__restrict__ xci,
                                                        const int32_t *__restrict__ yrp, int32_t *__restrict__ cnt,
                                                        int32_t *__restrict__ long_pad) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
        int64_t c = 0;
        for (int k = xrp[i]; k < xrp[i + 1]; ++k) c += yrp[xci[k] + 1] - yrp[xci[k]];
        cnt[i] = (int32_t)std::min<int64_t>(c, 0x7fffffff);
        int64_t p = 1;
        while (p < c) p <<= 1;
        long_pad[i] = c <= kSgCap ? 0 : p > 0x40000000 ? 0x7fffffff : (int32_t)p;   // (0x7fffffff: no scratch can hold it)
    }
}

enum SgMode { SG_COUNT = 0, SG_NUMERIC = 1 };
enum SgEpi { SG_PLAIN = 0, SG_SMOOTH = 1 };   // SG_SMOOTH: c_ij = [j == agg_i] t_i - (omega dinv_i) (X Y)_ij  (P from A and T)

template <int MODE, int EPI>
__global__ __launch_bounds__(64) void k_spgemm(int64_t m, const int32_t *__restrict__ xrp, const int32_t *__restrict__ xci,
                                               const double *__restrict__ xv, const int32_t *__restrict__ yrp,
                                               const int32_t *__restrict__ yci, const double *__restrict__ yv,
                                               const int32_t *__restrict__ cnt, const int32_t *__restrict__ long_off,
                                               uint64_t *__restrict__ gkey, double *__restrict__ gval,
                                               const int32_t *__restrict__ crp, int32_t *__restrict__ cci, double *__restrict__ cv,
                                               int32_t *__restrict__ rowlen, const int32_t *__restrict__ agg,
                                               const double *__restrict__ tval, const double *__restrict__ dinv, double omega) {
    __shared__ uint64_t skey[kSgCap];
    __shared__ double sval[kSgCap];
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
        const int c = cnt[i];
        uint64_t *key = skey;
        double *val = sval;
        if (c > kSgCap) {
            key = gkey + long_off[i];
            val = gval + long_off[i];
        }
        int m2 = 1;
        while (m2 < c) m2 <<= 1;
        // expand in product order
        int base = 0;
        for (int kk = xrp[i]; kk < xrp[i + 1]; ++kk) {
            const int k = xci[kk];
            const double xk = MODE == SG_NUMERIC ? xv[kk] : 0.0;
            const int y0 = yrp[k], len = yrp[k + 1] - y0;
            for (int t = lane; t < len; t += 64) {
                key[base + t] = ((uint64_t)(uint32_t)yci[y0 + t] << 32) | (uint32_t)(base + t);
                if (MODE == SG_NUMERIC) val[base + t] = xk * yv[y0 + t];
            }
            base += len;
        }
        for (int t = c + lane; t < m2; t += 64) key[t] = ~0ull;
        __syncthreads();
        // bitonic sort of key (val carried along)
        for (int size = 2; size <= m2; size <<= 1) {
            for (int half = size >> 1; half > 0; half >>= 1) {
                for (int t = lane; t < m2; t += 64) {
                    const int u = t ^ half;
                    if (u > t) {
                        const bool up = (t & size) == 0;
                        const uint64_t a = key[t], b = key[u];
                        if ((a > b) == up) {
                            key[t] = b;
                            key[u] = a;
                            if (MODE == SG_NUMERIC) {
                                const double va = val[t];
                                val[t] = val[u];
                                val[u] = va;
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        // compress: one output entry per distinct column
        int off = 0;
        const int out0 = MODE == SG_NUMERIC ? crp[i] : 0;
        for (int j0 = 0; j0 < c; j0 += 64) {
            const int j = j0 + lane;
            const bool head = j < c && (j == 0 || (key[j] >> 32) != (key[j - 1] >> 32));
            const unsigned long long mask = __ballot(head);
            if (MODE == SG_NUMERIC && head) {
                const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
                const uint32_t col = (uint32_t)(key[j] >> 32);
                double sum = val[j];
                for (int q = j + 1; q < c && (uint32_t)(key[q] >> 32) == col; ++q) sum += val[q];
                double out = sum;
                if (EPI == SG_SMOOTH) out = ((int)col == agg[i] ? tval[i] : 0.0) - (omega * dinv[i]) * sum;
                cci[out0 + pos] = (int32_t)col;
                cv[out0 + pos] = out;
            }
            off += __popcll(mask);
        }
        if (MODE == SG_COUNT && lane == 0) rowlen[i] = off;
        __syncthreads();
    }
}

__global__ void k_set_last(int32_t *rp, int64_t n) { rp[n] = 0; }

// *total += sum of v[0 .. n) in 64 bits (integers: the order does not matter): what an int32 scan of v would wrap on
__global__ __launch_bounds__(kBlock) void k_sum_i64(int64_t n, const int32_t *__restrict__ v, unsigned long long *total) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    unsigned long long t = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) t += (unsigned long long)(uint32_t)v[i];
    if (t) atomicAdd(total, t);
}

// ---- apply kernels ------------------------------------------------------------------------------------------------------
enum AmgOp { OP_PRE = 0, OP_SWEEP = 1, OP_POST = 2, OP_ACC = 3, OP_PLAIN = 4, OP_RES = 5 };

// One row per TPR lanes.  y_j is what the row gathers:
//   PRE    y_j = omega dinv_j b_j;         x_i = y_i,  r_i = b_i - sum a_ij y_j
//   SWEEP  y_j = x_j + omega dinv_j r_j;   x'_i = y_i, r'_i = b_i - sum a_ij y_j
//   POST   y_j = x_j;                      x'_i = x_i + omega dinv_i (b_i - sum a_ij y_j)   [part: <b, x'> per workgroup]
//   ACC    y_j = u_j;                      x'_i = x_i + sum a_ij y_j          (a = P)
//   PLAIN  y_j = u_j;                      x'_i = sum a_ij y_j                (a = P^T)
//   RES    y_j = x_j;                      r_i = b_i - sum a_ij y_j
// Storage types (all double: the fp64 cycle): AT the matrix values and dinv, BT b, WT the work vectors gathered (xin, rin, u) and
// r', OT x' (POST on level 0: z, double; otherwise WT).  Arithmetic is double; rnd<T> rounds what is stored as T where it is computed.
template <typename T>
__device__ __forceinline__ double rnd(double v) {
    return (double)(T)v;
}

template <int OP, int TPR, typename AT = double, typename BT = double, typename WT = double, typename OT = double>
__global__ __launch_bounds__(kBlock) void k_amg_row(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const AT *__restrict__ av, const AT *__restrict__ dinv, double omega,
                                                    const BT *__restrict__ b, const WT *__restrict__ xin,
                                                    const WT *__restrict__ rin, const WT *__restrict__ u,
                                                    OT *__restrict__ xout, WT *__restrict__ rout, double *__restrict__ part,
                                                    const int *__restrict__ done) {
    if (done && *done) return;        // (in the PCG loop: the updates enqueued beyond convergence cost a launch each, not a cycle)
    constexpr int RPB = kBlock / TPR;
    const int sub = threadIdx.x % TPR;
    double acc = 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < n; row0 += (int64_t)gridDim.x * RPB) {
        const int64_t i = row0 + threadIdx.x / TPR;
        double s = 0.0;
        if (i < n) {
            for (int k = rp[i] + sub; k < rp[i + 1]; k += TPR) {
                const int j = ci[k];
                double y;
                if (OP == OP_PRE) y = rnd<WT>(omega * dinv[j] * b[j]);
                else if (OP == OP_SWEEP) y = rnd<WT>(xin[j] + omega * dinv[j] * rin[j]);
                else if (OP == OP_POST || OP == OP_RES) y = xin[j];
                else y = u[j];
                s += av[k] * y;
            }
        }
#pragma unroll
        for (int w = 1; w < TPR; w <<= 1) s += __shfl_xor(s, w, TPR);
        if (i < n && sub == 0) {
            if (OP == OP_PRE) {
                xout[i] = (OT)(omega * dinv[i] * b[i]);
                rout[i] = (WT)(b[i] - s);
            } else if (OP == OP_SWEEP) {
                xout[i] = (OT)(xin[i] + omega * dinv[i] * rin[i]);
                rout[i] = (WT)(b[i] - s);
            } else if (OP == OP_POST) {
                const double x = rnd<OT>(xin[i] + omega * dinv[i] * (b[i] - s));
                xout[i] = (OT)x;
                if (part) acc += b[i] * x;
            } else if (OP == OP_ACC) {
                xout[i] = (OT)(xin[i] + s);
            } else if (OP == OP_RES) {
                rout[i] = (WT)(b[i] - s);
            } else {
                xout[i] = (OT)s;
            }
        }
    }
    if (OP == OP_POST && part) {   // fixed-order workgroup sum (rows are owned by lanes sub == 0; the others hold 0)
        __shared__ double red[kBlock / 64];
        const double w = wave_sum(acc);
        if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int q = 0; q < kBlock / 64; ++q) t += red[q];
            part[blockIdx.x] = t;
        }
    }
}

// One Gauss-Seidel colour pass: the rows rows[0 .. cnt) (one colour: no two share an edge) updated in place,
// x_i += dinv_i (b_i - sum_j a_ij x_j).  INIT (the first pass from x = 0): rows[0 .. n_all) are walked, the colour's own rows get
// dinv_i b_i and every other row 0.
template <int TPR, bool INIT>
__global__ __launch_bounds__(kBlock) void k_amg_gs(int64_t cnt, int64_t n_all, const int32_t *__restrict__ rows,
                                                   const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                   const double *__restrict__ av, const double *__restrict__ dinv,
                                                   const double *__restrict__ b, double *x, const int *__restrict__ done) {
    if (done && *done) return;
    constexpr int RPB = kBlock / TPR;
    const int sub = threadIdx.x % TPR;
    const int64_t total = INIT ? n_all : cnt;
    for (int64_t p0 = (int64_t)blockIdx.x * RPB; p0 < total; p0 += (int64_t)gridDim.x * RPB) {
        const int64_t p = p0 + threadIdx.x / TPR;
        if (INIT) {
            if (p < total && sub == 0) {
                const int i = rows[p];
                x[i] = p < cnt ? dinv[i] * b[i] : 0.0;
            }
            continue;
        }
        const int i = p < total ? rows[p] : 0;
        double s = 0.0;
        if (p < total)
            for (int k = rp[i] + sub; k < rp[i + 1]; k += TPR) s += av[k] * x[ci[k]];
#pragma unroll
        for (int w = 1; w < TPR; w <<= 1) s += __shfl_xor(s, w, TPR);
        if (p < total && sub == 0) x[i] = x[i] + dinv[i] * (b[i] - s);
    }
}

// `sweeps` symmetric sweeps of one level in ONE workgroup (a block barrier between colours, no grid-wide wait); init: from x = 0
template <int TPR>
__global__ __launch_bounds__(kGsBlockThreads) void k_amg_gs_block(int64_t n, int m, const int32_t *__restrict__ off,
                                                                  const int32_t *__restrict__ rows, const int32_t *__restrict__ rp,
                                                                  const int32_t *__restrict__ ci, const double *__restrict__ av,
                                                                  const double *__restrict__ dinv, const double *__restrict__ b,
                                                                  double *x, int sweeps, int init, const int *__restrict__ done) {
    if (done && *done) return;
    constexpr int RPB = kGsBlockThreads / TPR;
    const int sub = threadIdx.x % TPR;
    if (init) {
        for (int64_t i = threadIdx.x; i < n; i += kGsBlockThreads) x[i] = 0.0;
        __syncthreads();
    }
    for (int sw = 0; sw < sweeps; ++sw)
        for (int q = 0; q < 2 * m - 1; ++q) {
            const int c = q < m ? q : 2 * m - 2 - q;
            const int lo = off[c], hi = off[c + 1];
            for (int p0 = lo; p0 < hi; p0 += RPB) {
                const int p = p0 + (int)threadIdx.x / TPR;
                const int i = p < hi ? rows[p] : 0;
                double s = 0.0;
                if (p < hi)
                    for (int k = rp[i] + sub; k < rp[i + 1]; k += TPR) s += av[k] * x[ci[k]];
#pragma unroll
                for (int w = 1; w < TPR; w <<= 1) s += __shfl_xor(s, w, TPR);
                if (p < hi && sub == 0) x[i] = x[i] + dinv[i] * (b[i] - s);
            }
            __syncthreads();
        }
}

// One Chebyshev step on (x, r = b - A x): d' = c1 d + c2 (dinv r) (din null: the first step, d' = c2 (dinv r)), x' = x + d'
// (xin null: x = 0).  STEP gathers the new x_j on the fly and writes x', d' and r' = b - A x'; LAST writes x' only (part: <b, x'>
// per workgroup, rows owned as in k_amg_row so the partials line up with amg_rz_partials).
// Storage types as k_amg_row's: STEP stores d', x' and r' as WT, so d' is rounded before it enters x' = x + d' and x' before it enters
// the row sum; LAST stores only x' (as OT), so its d' is not rounded.  RT: the storage of r (pre-smoothing's first step reads r = b).
enum ChebMode { CHEB_STEP = 0, CHEB_LAST = 1 };
template <int TPR, int MODE, typename AT = double, typename BT = double, typename WT = double, typename OT = double,
          typename RT = WT>
__global__ __launch_bounds__(kBlock) void k_amg_cheb(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                     const AT *__restrict__ av, const AT *__restrict__ dinv,
                                                     const BT *__restrict__ b, const WT *__restrict__ xin,
                                                     const WT *__restrict__ din, const RT *__restrict__ rin, double c1, double c2,
                                                     OT *__restrict__ xout, WT *__restrict__ dout, WT *__restrict__ rout,
                                                     double *__restrict__ part, const int *__restrict__ done) {
    if (done && *done) return;
    constexpr int RPB = kBlock / TPR;
    const int sub = threadIdx.x % TPR;
    auto dnew = [&](int64_t j) {
        // (dinv r in double also when both are stored as float)
        const double d = din ? c1 * din[j] + c2 * ((double)dinv[j] * (double)rin[j]) : c2 * ((double)dinv[j] * (double)rin[j]);
        return MODE == CHEB_STEP ? rnd<WT>(d) : d;
    };
    auto xnew = [&](int64_t j, double d) { return rnd<OT>((xin ? xin[j] : 0.0) + d); };
    double acc = 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < n; row0 += (int64_t)gridDim.x * RPB) {
        const int64_t i = row0 + threadIdx.x / TPR;
        double s = 0.0;
        if (MODE == CHEB_STEP) {
            if (i < n)
                for (int k = rp[i] + sub; k < rp[i + 1]; k += TPR) {
                    const int j = ci[k];
                    s += av[k] * xnew(j, dnew(j));
                }
#pragma unroll
            for (int w = 1; w < TPR; w <<= 1) s += __shfl_xor(s, w, TPR);
        }
        if (i < n && sub == 0) {
            const double d = dnew(i);
            const double x = xnew(i, d);
            xout[i] = (OT)x;
            if (MODE == CHEB_STEP) {
                dout[i] = (WT)d;
                rout[i] = (WT)(b[i] - s);
            } else if (part) {
                acc += b[i] * x;
            }
        }
    }
    if (MODE == CHEB_LAST && part) {
        __shared__ double red[kBlock / 64];
        const double w = wave_sum(acc);
        if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int q = 0; q < kBlock / 64; ++q) t += red[q];
            part[blockIdx.x] = t;
        }
    }
}

// x = C b, C dense row-major (nc x nc): one wave per row, fixed-order sums (VT: the storage of b and x; C and the sums are double)
template <typename VT = double>
__global__ __launch_bounds__(kBlock) void k_amg_gemv(int64_t nc, const double *__restrict__ C, const VT *__restrict__ b,
                                                     VT *__restrict__ x, const int *__restrict__ done) {
    if (done && *done) return;
    const int lane = threadIdx.x & 63;
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; i < nc; i += ((int64_t)gridDim.x * kBlock) >> 6) {
        double s = 0.0;
        for (int64_t j = lane; j < nc; j += 64) s += C[i * nc + j] * b[j];
        s = wave_sum(s);
        if (lane == 63) x[i] = (VT)s;
    }
}

// dst[k] = (float) src[order ? order[k] : k] (round to nearest even): the fp32 copies of the cycle's operands
__global__ __launch_bounds__(kBlock) void k_amg_to_f32(int64_t n, const double *__restrict__ src, const int32_t *__restrict__ order,
                                                       float *__restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) dst[k] = (float)src[order ? order[k] : k];
}

int tpr_for(const CsrDev &A) {
    const double mean = A.n > 0 ? (double)A.nnz / (double)A.n : 1.0;
    int tpr = 2;                      // the planner's rule for its CSR-vector kernel (make_plan)
    while (tpr < 64 && 2 * tpr < mean) tpr *= 2;
    return tpr;
}

// (av: the values the rows multiply -- A.val, or its fp32 copy)
template <int OP, typename AT, typename BT, typename WT, typename OT>
void launch_row(const CsrDev &A, const AT *av, int tpr, const AT *dinv, double omega, const BT *b, const WT *xin, const WT *rin,
                const WT *u, OT *xout, WT *rout, double *part, int *grid_out, hipStream_t s, const int *done) {
    const int rpb = kBlock / tpr;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((A.n + rpb - 1) / rpb, kApplyMaxGrid));
    if (grid_out) *grid_out = grid;
#define AMG_ROW(T)                                                                                                           \
    case T:                                                                                                                  \
        hipLaunchKernelGGL((k_amg_row<OP, T, AT, BT, WT, OT>), dim3(grid), dim3(kBlock), 0, s, A.n, A.rowptr, A.col, av, dinv, \
                           omega, b, xin, rin, u, xout, rout, part, done);                                                   \
        break;
    switch (tpr) { AMG_ROW(2) AMG_ROW(4) AMG_ROW(8) AMG_ROW(16) AMG_ROW(32) default: AMG_ROW(64) }
#undef AMG_ROW
}

void launch_gs(const AmgLevel &L, int64_t lo, int64_t cnt, bool init, const double *b, double *x, hipStream_t s, const int *done) {
    const int rpb = kBlock / L.tpr_a;
    const int64_t total = init ? L.A.n : cnt;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + rpb - 1) / rpb, kApplyMaxGrid));
    const int32_t *rows = L.gs_rows + lo;
#define AMG_GS(T)                                                                                                              \
    case T:                                                                                                                    \
        if (init)                                                                                                              \
            hipLaunchKernelGGL((k_amg_gs<T, true>), dim3(grid), dim3(kBlock), 0, s, cnt, L.A.n, rows, L.A.rowptr, L.A.col,       \
                               L.A.val, L.dinv, b, x, done);                                                                   \
        else                                                                                                                   \
            hipLaunchKernelGGL((k_amg_gs<T, false>), dim3(grid), dim3(kBlock), 0, s, cnt, L.A.n, rows, L.A.rowptr, L.A.col,      \
                               L.A.val, L.dinv, b, x, done);                                                                   \
        break;
    switch (L.tpr_a) { AMG_GS(2) AMG_GS(4) AMG_GS(8) AMG_GS(16) AMG_GS(32) default: AMG_GS(64) }
#undef AMG_GS
}

void launch_gs_block(const AmgLevel &L, int sweeps, bool init, const double *b, double *x, hipStream_t s, const int *done) {
    const int m = (int)L.gs_off.size() - 1;
#define AMG_GSB(T)                                                                                                             \
    case T:                                                                                                                    \
        hipLaunchKernelGGL((k_amg_gs_block<T>), dim3(1), dim3(kGsBlockThreads), 0, s, L.A.n, m, L.gs_off_dev, L.gs_rows,       \
                           L.A.rowptr, L.A.col, L.A.val, L.dinv, b, x, sweeps, init ? 1 : 0, done);                            \
        break;
    switch (L.tpr_a) { AMG_GSB(2) AMG_GSB(4) AMG_GSB(8) AMG_GSB(16) AMG_GSB(32) default: AMG_GSB(64) }
#undef AMG_GSB
}

// `sweeps` symmetric Gauss-Seidel sweeps of level L on x (init: from x = 0); returns the launches
int gs_sweeps(const AmgLevel &L, int sweeps, bool init, const double *b, double *x, hipStream_t s, const int *done) {
    if (L.gs_block) {
        launch_gs_block(L, sweeps, init, b, x, s, done);
        return 1;
    }
    const int m = (int)L.gs_off.size() - 1;
    int k = 0;
    for (int sw = 0; sw < sweeps; ++sw)
        for (int q = 0; q < 2 * m - 1; ++q, ++k) {
            const int c = q < m ? q : 2 * m - 2 - q;
            launch_gs(L, L.gs_off[c], L.gs_off[c + 1] - L.gs_off[c], init && k == 0, b, x, s, done);
        }
    return k;
}

template <int MODE, typename AT, typename BT, typename WT, typename OT, typename RT>
void launch_cheb(const AmgLevel &L, const AT *av, const AT *dinv, double c1, double c2, const BT *b, const WT *xin, const WT *din,
                 const RT *rin, OT *xout, WT *dout, WT *rout, double *part, int *grid_out, hipStream_t s, const int *done) {
    const int rpb = kBlock / L.tpr_a;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((L.A.n + rpb - 1) / rpb, kApplyMaxGrid));
    if (grid_out) *grid_out = grid;
#define AMG_CHEB(T)                                                                                                            \
    case T:                                                                                                                    \
        hipLaunchKernelGGL((k_amg_cheb<T, MODE, AT, BT, WT, OT, RT>), dim3(grid), dim3(kBlock), 0, s, L.A.n, L.A.rowptr, L.A.col,  \
                           av, dinv, b, xin, din, rin, c1, c2, xout, dout, rout, part, done);                                  \
        break;
    switch (L.tpr_a) { AMG_CHEB(2) AMG_CHEB(4) AMG_CHEB(8) AMG_CHEB(16) AMG_CHEB(32) default: AMG_CHEB(64) }
#undef AMG_CHEB
}

// ---- host helpers ---------------------------------------------------------------------------------------------------
void free_level(AmgLevel &L, bool keep_a) {
    if (!keep_a) free_csr(L.A);
    dev_free(L.dinv);
    dev_free(L.strong);
    dev_free(L.roots);
    dev_free(L.agg);
    free_csr(L.P);
    free_csr(L.Pt);
    free_csr(L.AP);
    dev_free(L.pt_order);
    dev_free(L.b); dev_free(L.xa); dev_free(L.xb); dev_free(L.ra); dev_free(L.rb);
    dev_free(L.gs_rows); dev_free(L.gs_off_dev);
    dev_free(L.da); dev_free(L.db);
    dev_free(L.a32); dev_free(L.p32); dev_free(L.pt32); dev_free(L.dinv32);
    dev_free(L.b32); dev_free(L.xa32); dev_free(L.xb32); dev_free(L.ra32); dev_free(L.rb32); dev_free(L.da32); dev_free(L.db32);
    L = AmgLevel();
}

// an owned CSR matrix that is freed unless released (a Galerkin product in flight between two levels)
struct CsrOwner {
    CsrDev c;
    ~CsrOwner() { free_csr(c); }
};

// C = X Y (X: m rows, Y: ncols columns).  C.rowptr / C.col given (same pattern as before): numeric pass only.
int spgemm(const CsrDev &X, const CsrDev &Y, int64_t ncols, CsrDev &C, int epi, const int32_t *agg, const double *tval,
           const double *dinv, double omega, hipStream_t s) {
    const int64_t m = X.n;
    DevBuf<int32_t> cnt, lpad, loff, len;
    DevBuf<unsigned long long> total;
    DPCG_TRY(cnt.alloc(m));
    DPCG_TRY(lpad.alloc(m + 1));
    DPCG_TRY(loff.alloc(m + 1));
    DPCG_TRY(total.alloc(1));
    hipLaunchKernelGGL(k_sg_products, dim3(grid_blocks(m, kAmgGrid)), dim3(kBlock), 0, s, m, X.rowptr, X.col, Y.rowptr, cnt.p, lpad.p);
    hipLaunchKernelGGL(k_set_last, dim3(1), dim3(1), 0, s, lpad.p, m);
    // the scratch offsets are an int32 scan: its total is checked in 64 bits first (a sum past 2^32 would wrap back to a small
    // positive number, and the long rows would be sorted outside the scratch)
    DPCG_HIP(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_sum_i64, dim3(grid_blocks(m, kAmgGrid)), dim3(kBlock), 0, s, m, lpad.p, total.p);
    unsigned long long scratch64 = 0;
    DPCG_TRY(fetch(&scratch64, total.p, 1, s));
    if (scratch64 >= 0x7fffffffull) {
        set_error("dpcg_set_precond_amg: the long rows of a Galerkin product need more than 2^31 scratch entries");
        return DPCG_ERR_INVALID;
    }
    DPCG_TRY(exclusive_scan_i32(lpad.p, loff.p, m + 1, s));
    const int32_t scratch = (int32_t)scratch64;
    DevBuf<uint64_t> gkey;
    DevBuf<double> gval;
    DPCG_TRY(gkey.alloc(std::max<int64_t>(1, scratch)));
    DPCG_TRY(gval.alloc(std::max<int64_t>(1, scratch)));
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(m, 1 << 20));
    const bool symbolic = C.rowptr == nullptr;
    if (symbolic) {
        C = CsrDev();
        C.n = m;
        C.owned = true;
        DPCG_TRY(len.alloc(m + 1));
        DPCG_TRY(dev_alloc(&C.rowptr, m + 1));
        hipLaunchKernelGGL((k_spgemm<SG_COUNT, SG_PLAIN>), dim3(grid), dim3(64), 0, s, m, X.rowptr, X.col, X.val, Y.rowptr, Y.col,
                           Y.val, cnt.p, loff.p, gkey.p, gval.p, nullptr, nullptr, nullptr, len.p, nullptr, nullptr, nullptr, 0.0);
        hipLaunchKernelGGL(k_set_last, dim3(1), dim3(1), 0, s, len.p, m);
        DPCG_HIP(hipMemsetAsync(total.p, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_sum_i64, dim3(grid_blocks(m, kAmgGrid)), dim3(kBlock), 0, s, m, len.p, total.p);
        unsigned long long nnz64 = 0;
        DPCG_TRY(fetch(&nnz64, total.p, 1, s));
        if (nnz64 > 0x7fffffffull) {
            set_error("dpcg_set_precond_amg: a Galerkin product has more than 2^31 entries");
            return DPCG_ERR_INVALID;
        }
        DPCG_TRY(exclusive_scan_i32(len.p, C.rowptr, m + 1, s));
        const int32_t nnz = (int32_t)nnz64;
        C.nnz = nnz;
        DPCG_TRY(dev_alloc(&C.col, std::max<int64_t>(1, nnz)));
        DPCG_TRY(dev_alloc(&C.val, std::max<int64_t>(1, nnz)));
    }
    (void)ncols;
    if (epi == SG_SMOOTH)
        hipLaunchKernelGGL((k_spgemm<SG_NUMERIC, SG_SMOOTH>), dim3(grid), dim3(64), 0, s, m, X.rowptr, X.col, X.val, Y.rowptr, Y.col,
                           Y.val, cnt.p, loff.p, gkey.p, gval.p, C.rowptr, C.col, C.val, nullptr, agg, tval, dinv, omega);
    else
        hipLaunchKernelGGL((k_spgemm<SG_NUMERIC, SG_PLAIN>), dim3(grid), dim3(64), 0, s, m, X.rowptr, X.col, X.val, Y.rowptr, Y.col,
                           Y.val, cnt.p, loff.p, gkey.p, gval.p, C.rowptr, C.col, C.val, nullptr, nullptr, nullptr, nullptr, 0.0);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// P^T (nc x n); `order` (entry of P^T -> entry of P) kept for a values-only refresh
int transpose_p(const CsrDev &P, int64_t nc, CsrDev &Pt, int32_t **order_io, hipStream_t s) {
    const int64_t nnz = P.nnz;
    if (*order_io) {
        launch_gather_f64(nnz, *order_io, P.val, Pt.val, s);
    } else {
        DPCG_TRY(dev_alloc(order_io, nnz));
        free_csr(Pt);
        Pt.n = nc;
        Pt.nnz = nnz;
        Pt.owned = true;
        DPCG_TRY(dev_alloc(&Pt.rowptr, nc + 1));
        DPCG_TRY(dev_alloc(&Pt.col, nnz));
        DPCG_TRY(dev_alloc(&Pt.val, nnz));
        DPCG_TRY(transpose_csr(P.n, nc, nnz, P.rowptr, P.col, P.val, Pt.rowptr, Pt.col, Pt.val, *order_io, s));
    }
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// rho = theta_max + err_max of a kRhoSteps-step Lanczos estimate of the spectrum of D^-1 A_l, on a handle that borrows A_l
int estimate_rho(const CsrDev &A, const int32_t *perm, uint64_t seed, double *rho, hipStream_t s) {
    dpcg_handle_t t = nullptr;
    DPCG_TRY(dpcg_create(&t, A.n, A.nnz, A.rowptr, A.col, A.val, DPCG_F64, DPCG_DEVICE, 0, (dpcg_stream_t)s));
    int st = dpcg_set_precond_jacobi(t, nullptr, DPCG_DEVICE, (dpcg_stream_t)s);
    int steps = 0;
    double tmin = 0, tmax = 0, emin = 0, emax = 0;
    if (st >= 0) {
        t->perm = const_cast<int32_t *>(perm);       // (the start vector hashes the caller's row index)
        st = dpcg_spectrum(t, kRhoSteps, 0.0, seed, (dpcg_stream_t)s, &steps, &tmin, &tmax, &emin, &emax, nullptr, nullptr);
        t->perm = nullptr;
    }
    dpcg_destroy(t);
    if (st < 0) return st;
    if (st == DPCG_BREAKDOWN || !(tmax > 0.0) || !std::isfinite(tmax + emax)) {
        set_error("dpcg_set_precond_amg: the spectral-radius estimate of D^-1 A broke down (A is not symmetric positive definite)");
        return DPCG_ERR_PIVOT;
    }
    *rho = tmax + emax;
    return DPCG_OK;
}

// Dense inverse of the coarsest matrix by Cholesky on the host
int coarse_inverse(const CsrDev &A, int level, double **cinv, hipStream_t s) {
    const int64_t n = A.n;
    std::vector<int32_t> rp(n + 1), ci(A.nnz);
    std::vector<double> v(A.nnz);
    DPCG_HIP(hipMemcpyAsync(rp.data(), A.rowptr, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipMemcpyAsync(ci.data(), A.col, A.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipMemcpyAsync(v.data(), A.val, A.nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    std::vector<double> L((size_t)n * n, 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int k = rp[i]; k < rp[i + 1]; ++k) L[(size_t)i * n + ci[k]] += v[k];
    for (int64_t j = 0; j < n; ++j) {                  // in place, lower triangle
        double d = L[(size_t)j * n + j];
        for (int64_t k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) {
            char buf[200];
            snprintf(buf, sizeof(buf), "dpcg_set_precond_amg: the coarsest matrix (level %d, %lld rows) is not positive definite "
                     "(pivot %lld)", level, (long long)n, (long long)j);
            set_error(buf);
            return DPCG_ERR_PIVOT;
        }
        d = std::sqrt(d);
        L[(size_t)j * n + j] = d;
        for (int64_t i = j + 1; i < n; ++i) {
            double a = L[(size_t)i * n + j];
            for (int64_t k = 0; k < j; ++k) a -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = a / d;
        }
    }
    // W = L^-1 (lower triangular) row by row, W[i, :] = (e_i - sum_{k<i} L_ik W[k, :]) / L_ii, and C = W^T W accumulated row by
    // row of W: every inner loop runs along a contiguous row (n^3 / 6 multiply-adds each; a few seconds at the 4096-row limit)
    std::vector<double> W((size_t)n * n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        double *wi = &W[(size_t)i * n];
        wi[i] = 1.0;
        for (int64_t k = 0; k < i; ++k) {
            const double a = L[(size_t)i * n + k];
            if (a == 0.0) continue;
            const double *wk = &W[(size_t)k * n];
            for (int64_t j = 0; j <= k; ++j) wi[j] -= a * wk[j];
        }
        const double d = L[(size_t)i * n + i];
        for (int64_t j = 0; j <= i; ++j) wi[j] /= d;
    }
    std::vector<double> C((size_t)n * n, 0.0);        // lower triangle of W^T W, then mirrored
    for (int64_t k = 0; k < n; ++k) {
        const double *wk = &W[(size_t)k * n];
        for (int64_t i = 0; i <= k; ++i) {
            const double a = wk[i];
            if (a == 0.0) continue;
            double *ci = &C[(size_t)i * n];
            for (int64_t j = 0; j <= i; ++j) ci[j] += a * wk[j];
        }
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < i; ++j) C[(size_t)j * n + i] = C[(size_t)i * n + j];
    DPCG_TRY(dev_alloc(cinv, n * n));
    DPCG_HIP(hipMemcpyAsync(*cinv, C.data(), (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// the work vectors of one level in the cycle's precision (the other set stays null)
template <typename W>
int alloc_work_t(AmgLevel &L, bool coarse, int sweeps, W *&b, W *&xa, W *&xb, W *&ra, W *&rb, W *&da, W *&db) {
    const int64_t n = L.A.n;
    DPCG_TRY(dev_alloc(&b, n));
    DPCG_TRY(dev_alloc(&xa, n));
    if (coarse) return DPCG_OK;
    DPCG_TRY(dev_alloc(&xb, n));
    DPCG_TRY(dev_alloc(&ra, n));
    if (sweeps > 1 || L.smoother == DPCG_AMG_CHEBYSHEV) DPCG_TRY(dev_alloc(&rb, n));
    if (L.smoother == DPCG_AMG_CHEBYSHEV) {
        DPCG_TRY(dev_alloc(&da, n));
        DPCG_TRY(dev_alloc(&db, n));
    }
    return DPCG_OK;
}

int alloc_work(AmgLevel &L, bool coarse, int sweeps, int precision) {
    if (precision == DPCG_AMG_FP32) return alloc_work_t(L, coarse, sweeps, L.b32, L.xa32, L.xb32, L.ra32, L.rb32, L.da32, L.db32);
    return alloc_work_t(L, coarse, sweeps, L.b, L.xa, L.xb, L.ra, L.rb, L.da, L.db);
}

// fp32 cycle: the values of A_l, P_l, P_l^T (the rounded numbers of P_l, through pt_order) and dinv_l once more, rounded to fp32
int make_f32_copies(AmgLevel &L, hipStream_t s) {
    const int64_t n = L.A.n, an = std::max<int64_t>(1, L.A.nnz), pn = std::max<int64_t>(1, L.P.nnz);
    DPCG_TRY(dev_alloc(&L.a32, an));
    DPCG_TRY(dev_alloc(&L.p32, pn));
    DPCG_TRY(dev_alloc(&L.pt32, pn));
    DPCG_TRY(dev_alloc(&L.dinv32, n));
    hipLaunchKernelGGL(k_amg_to_f32, dim3(grid_blocks(L.A.nnz, kAmgGrid)), dim3(kBlock), 0, s, L.A.nnz, L.A.val, nullptr, L.a32);
    hipLaunchKernelGGL(k_amg_to_f32, dim3(grid_blocks(L.P.nnz, kAmgGrid)), dim3(kBlock), 0, s, L.P.nnz, L.P.val, nullptr, L.p32);
    hipLaunchKernelGGL(k_amg_to_f32, dim3(grid_blocks(L.P.nnz, kAmgGrid)), dim3(kBlock), 0, s, L.P.nnz, L.P.val, L.pt_order, L.pt32);
    hipLaunchKernelGGL(k_amg_to_f32, dim3(grid_blocks(n, kAmgGrid)), dim3(kBlock), 0, s, n, L.dinv, nullptr, L.dinv32);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// Gauss-Seidel: colour level l (taken over from the parked level O when its pattern was kept; level 0: the handle's cached colouring,
// computed and cached here when there is none).  A graph the greedy colouring cannot colour with 63 colours keeps damped Jacobi.
int color_level(dpcg_system *h, AmgLevel &L, AmgLevel *O, int l, hipStream_t s) {
    const int64_t n = L.A.n;
    if (O && O->gs_rows && !O->gs_off.empty() && O->gs_off.back() == n) {
        L.gs_rows = O->gs_rows; O->gs_rows = nullptr;
        L.gs_off_dev = O->gs_off_dev; O->gs_off_dev = nullptr;
        L.gs_off.swap(O->gs_off);
    } else {
        const bool cached = l == 0 && h->mc_perm && (int)h->mc_offsets.size() == h->mc_colors + 1 && h->mc_offsets.back() == n;
        if (cached) {
            L.gs_off = h->mc_offsets;
            DPCG_TRY(dev_alloc(&L.gs_rows, n));
            DPCG_HIP(hipMemcpyAsync(L.gs_rows, h->mc_perm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        } else {
            int32_t *p = nullptr, *ip = nullptr;
            int nc = 0;
            std::vector<int32_t> off;
            const int st = multicolor_order(L.A, &p, &ip, &nc, s, &off);
            if (st == DPCG_ERR_INVALID) {             // more than 63 colours (or a pattern it cannot colour): damped Jacobi here
                dev_free(p);
                dev_free(ip);
                L.smoother = DPCG_AMG_JACOBI;
                return DPCG_OK;
            }
            DPCG_TRY(st);
            if (l == 0 && !h->mc_perm) {              // the handle keeps the colouring of its pattern (it survives update_values)
                DPCG_TRY(dev_alloc(&L.gs_rows, n));
                DPCG_HIP(hipMemcpyAsync(L.gs_rows, p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
                h->mc_perm = p;
                h->mc_iperm = ip;
                h->mc_colors = nc;
                h->mc_offsets = off;
            } else {
                L.gs_rows = p;
                dev_free(ip);
            }
            L.gs_off.swap(off);
        }
        DPCG_TRY(dev_alloc(&L.gs_off_dev, (int64_t)L.gs_off.size()));
        DPCG_HIP(hipMemcpyAsync(L.gs_off_dev, L.gs_off.data(), L.gs_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DPCG_HIP(hipStreamSynchronize(s));
    }
    L.smoother = DPCG_AMG_GAUSS_SEIDEL;
    L.gs_block = n <= gs_block_rows();
    return DPCG_OK;
}

// Chebyshev on [rho / eig_ratio, rho]: theta, delta, sigma and the coefficients of every step, in double on the host in this order
void chebyshev_coefficients(AmgLevel &L, int degree, double eig_ratio) {
    const double u = L.rho, lo = u / eig_ratio;
    const double theta = (u + lo) / 2.0, delta = (u - lo) / 2.0, sigma = theta / delta;
    L.cheb_lo = lo;
    L.cheb_hi = u;
    L.cheb_c1.assign(degree, 0.0);
    L.cheb_c2.assign(degree, 0.0);
    L.cheb_c2[0] = 1.0 / theta;
    double rho0 = 1.0 / sigma;
    for (int k = 1; k < degree; ++k) {
        const double rho1 = 1.0 / (2.0 * sigma - rho0);
        L.cheb_c1[k] = rho1 * rho0;
        L.cheb_c2[k] = 2.0 * rho1 / delta;
        rho0 = rho1;
    }
    L.smoother = DPCG_AMG_CHEBYSHEV;
}

void free_state(AmgState *S) {
    if (!S) return;
    for (AmgLevel &L : S->lv) free_level(L, false);
    S->lv.clear();
    dev_free(S->cinv);
}

int level_error(int status, int level, const char *what) {
    char buf[256];
    snprintf(buf, sizeof(buf), "dpcg_set_precond_amg: level %d: %s", level, what);
    set_error(buf);
    return status;
}

// MIS(2) of the strong graph of level L: L.roots (1 = root)
int mis2(AmgLevel &L, const int32_t *perm, uint64_t seed, int *flags, int8_t *st, uint64_t *hsh, int32_t *cid, hipStream_t s) {
    const int64_t n = L.A.n;
    DevBuf<int8_t> st2;
    DevBuf<int32_t> m1, m2;
    DPCG_TRY(st2.alloc(n));
    DPCG_TRY(m1.alloc(n));
    DPCG_TRY(m2.alloc(n));
    const int g = grid_blocks(n, kAmgGrid);
    for (int round = 0;; ++round) {
        if (round > 100000) return invalid("dpcg_set_precond_amg: MIS(2) did not terminate");
        hipLaunchKernelGGL(k_mis_max, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.strong, st, hsh, cid, nullptr, m1.p);
        hipLaunchKernelGGL(k_mis_max, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.strong, st, hsh, cid, m1.p, m2.p);
        DPCG_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_mis_update, dim3(g), dim3(kBlock), 0, s, n, st, m2.p, st2.p, flags);
        DPCG_HIP(hipMemcpyAsync(st, st2.p, (size_t)n, hipMemcpyDeviceToDevice, s));
        int left = 0;
        DPCG_TRY(fetch(&left, flags, 1, s));
        if (!left) break;
    }
    (void)perm;
    (void)seed;
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

// Build the hierarchy; `old` (may be null): a parked hierarchy of the same pattern and parameters, whose pattern-only parts are taken
// over: level by level, while the aggregates come out the same as the parked ones, the structures of P, A P, P^T (with its sort order)
// and A_{l+1}; only their values are computed again.  (The aggregates themselves are recomputed: the far rule looks at values, and an
// entry that cancels to zero leaves the strength graph.)
int build(dpcg_system *h, AmgState &S, AmgState *old, hipStream_t s) {
    PhaseTimer pt(s);
    DevBuf<int> flags;
    DPCG_TRY(flags.alloc(2));
    bool reuse = old != nullptr;
    CsrOwner next_owner;                            // A_{l+1} as the Galerkin product of level l left it (freed on an error return)
    CsrDev &nextA = next_owner.c;
    for (int l = 0;; ++l) {
        S.lv.emplace_back();
        AmgLevel &L = S.lv.back();
        AmgLevel *O = (reuse && l < (int)old->lv.size()) ? &old->lv[l] : nullptr;
        if (l == 0) {
            L.A = h->A;
            L.A.owned = false;
            L.A.val32 = nullptr;
        } else {
            L.A = nextA;
            nextA = CsrDev();
        }
        const int64_t n = L.A.n;
        const int g = grid_blocks(n, kAmgGrid);
        DevBuf<double> diag;
        DPCG_TRY(dev_alloc(&L.dinv, n));
        DPCG_TRY(diag.alloc(n));
        DPCG_HIP(hipMemsetAsync(flags.p, 0, 2 * sizeof(int), s));
        hipLaunchKernelGGL(k_amg_diag, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.A.val, L.dinv, diag.p, flags.p);
        int bad = 0;
        DPCG_TRY(fetch(&bad, flags.p, 1, s));
        if (bad) return level_error(DPCG_ERR_PIVOT, l, "a diagonal entry is missing, zero, negative or not finite");
        bool coarsest = n <= S.max_coarse || l == S.max_levels - 1;
        DevBuf<int32_t> cid, flag_by_cid, rank;
        int64_t nc = 0;
        if (!coarsest) {
            DPCG_TRY(dev_alloc(&L.strong, std::max<int64_t>(1, L.A.nnz)));
            hipLaunchKernelGGL(k_amg_strength, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.A.val, diag.p, S.theta, L.strong);
            DevBuf<int8_t> st;
            DevBuf<uint64_t> hsh;
            DPCG_TRY(st.alloc(n));
            DPCG_TRY(hsh.alloc(n));
            DPCG_TRY(cid.alloc(n));
            const int32_t *perm = l == 0 ? h->perm : nullptr;
            hipLaunchKernelGGL(k_mis_init, dim3(g), dim3(kBlock), 0, s, n, (unsigned long long)S.seed, perm, st.p, hsh.p, cid.p);
            DPCG_TRY(flag_by_cid.alloc(n + 1));
            DPCG_TRY(rank.alloc(n + 1));
            DPCG_TRY(dev_alloc(&L.roots, n));
            DPCG_TRY(mis2(L, perm, S.seed, flags.p, st.p, hsh.p, cid.p, s));
            hipLaunchKernelGGL(k_root_flags, dim3(g), dim3(kBlock), 0, s, n, st.p, cid.p, L.roots, flag_by_cid.p);
            hipLaunchKernelGGL(k_set_last, dim3(1), dim3(1), 0, s, flag_by_cid.p, n);
            DPCG_TRY(exclusive_scan_i32(flag_by_cid.p, rank.p, n + 1, s));
            int32_t nc32 = 0;
            DPCG_TRY(fetch(&nc32, rank.p + n, 1, s));
            nc = nc32;
            if (nc <= 0 || (double)nc > 0.9 * (double)n) coarsest = true;      // coarsening stalls
            pt.mark("amg: strength + MIS(2)");
        }
        if (coarsest) {
            dev_free(L.strong);
            dev_free(L.roots);
            if (n > 4096) {
                char buf[200];
                snprintf(buf, sizeof(buf), "the coarsest level has %lld rows (at most 4096 are solved densely): raise max_levels or "
                         "max_coarse's reach", (long long)n);
                return level_error(DPCG_ERR_INVALID, l, buf);
            }
            DPCG_TRY(coarse_inverse(L.A, l, &S.cinv, s));
            S.nco = n;
            DPCG_TRY(alloc_work(L, true, S.sweeps, S.precision));
            pt.mark("amg: coarse inverse");
            break;
        }
        L.nc = nc;
        // aggregates
        DevBuf<int32_t> agg1;
        DPCG_TRY(agg1.alloc(n));
        DPCG_TRY(dev_alloc(&L.agg, n));
        hipLaunchKernelGGL(k_agg_near, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.strong, L.roots, cid.p, rank.p, agg1.p);
        DPCG_HIP(hipMemsetAsync(flags.p, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_agg_far, dim3(g), dim3(kBlock), 0, s, n, L.A.rowptr, L.A.col, L.A.val, L.strong, cid.p, agg1.p, L.agg, flags.p);
        DPCG_TRY(fetch(&bad, flags.p, 1, s));
        if (bad) return level_error(DPCG_ERR_STATE, l, "a row was left without an aggregate");
        bool same = false;
        if (O && O->agg && O->nc == nc && O->P.rowptr) {
            DPCG_HIP(hipMemsetAsync(flags.p, 0, sizeof(int), s));
            hipLaunchKernelGGL(k_diff_i32, dim3(g), dim3(kBlock), 0, s, n, L.agg, O->agg, flags.p);
            int diff = 1;
            DPCG_TRY(fetch(&diff, flags.p, 1, s));
            same = diff == 0 && l + 1 < (int)old->lv.size() && old->lv[l + 1].A.rowptr;
        }
        if (same) {                                 // the pattern of P, A P, P^T and A_{l+1} is the parked one: values only
            ++S.reused_levels;
            L.P = O->P; O->P = CsrDev();
            L.AP = O->AP; O->AP = CsrDev();
            L.Pt = O->Pt; O->Pt = CsrDev();
            L.pt_order = O->pt_order; O->pt_order = nullptr;
            nextA = old->lv[l + 1].A; old->lv[l + 1].A = CsrDev();
        } else {
            reuse = false;
        }
        // tentative prolongator and the spectral radius of D^-1 A
        CsrOwner t_owner;
        CsrDev &T = t_owner.c;
        DevBuf<int32_t> size;
        DPCG_TRY(size.alloc(nc));
        T.owned = true;
        DPCG_TRY(dev_alloc(&T.rowptr, n + 1));
        DPCG_TRY(dev_alloc(&T.col, n));
        DPCG_TRY(dev_alloc(&T.val, n));
        T.n = n;
        T.nnz = n;
        DPCG_HIP(hipMemsetAsync(size.p, 0, (size_t)nc * sizeof(int32_t), s));
        hipLaunchKernelGGL(k_agg_size, dim3(g), dim3(kBlock), 0, s, n, L.agg, size.p);
        hipLaunchKernelGGL(k_tentative, dim3(grid_blocks(n + 1, kAmgGrid)), dim3(kBlock), 0, s, n, L.agg, size.p, T.rowptr, T.col, T.val);
        pt.mark("amg: aggregates");
        DPCG_TRY(estimate_rho(L.A, l == 0 ? h->perm : nullptr, S.seed, &L.rho, s));
        L.omega = (4.0 / 3.0) / L.rho;
        pt.mark("amg: rho (Lanczos)");
        // P = (I - omega D^-1 A) T, A P, P^T, A_{l+1} = P^T (A P)
        DPCG_TRY(spgemm(L.A, T, nc, L.P, SG_SMOOTH, L.agg, T.val, L.dinv, L.omega, s));
        DPCG_TRY(spgemm(L.A, L.P, nc, L.AP, SG_PLAIN, nullptr, nullptr, nullptr, 0.0, s));
        DPCG_TRY(transpose_p(L.P, nc, L.Pt, &L.pt_order, s));
        DPCG_TRY(spgemm(L.Pt, L.AP, nc, nextA, SG_PLAIN, nullptr, nullptr, nullptr, 0.0, s));
        pt.mark("amg: Galerkin product");
        L.tpr_a = tpr_for(L.A);
        L.tpr_p = tpr_for(L.P);
        L.tpr_pt = tpr_for(L.Pt);
        if (S.smoother == DPCG_AMG_GAUSS_SEIDEL) {
            DPCG_TRY(color_level(h, L, O, l, s));
            pt.mark("amg: colouring");
        } else if (S.smoother == DPCG_AMG_CHEBYSHEV) {
            chebyshev_coefficients(L, S.degree, S.eig_ratio);
        }
        DPCG_TRY(alloc_work(L, false, S.sweeps, S.precision));
        if (l == 0) {                               // (level 0's right-hand side is the caller's r)
            dev_free(L.b);
            dev_free(L.b32);
        }
        if (S.precision == DPCG_AMG_FP32) {
            DPCG_TRY(make_f32_copies(L, s));
            pt.mark("amg: fp32 copies");
        }
    }
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

void free_amg(AmgState *&S) {
    if (!S) return;
    free_state(S);
    delete S;
    S = nullptr;
}

int amg_launches(const AmgState *S) {
    if (!S) return 0;
    const int nu = S->sweeps;
    int t = 1;                                        // the coarse GEMV
    for (size_t l = 0; l + 1 < S->lv.size(); ++l) {
        const AmgLevel &L = S->lv[l];
        if (L.smoother == DPCG_AMG_GAUSS_SEIDEL)      // sweeps, residual, restriction, correction, sweeps
            t += L.gs_block ? 5 : 2 * nu * (2 * ((int)L.gs_off.size() - 1) - 1) + 3;
        else if (L.smoother == DPCG_AMG_CHEBYSHEV)    // steps, restriction, correction, residual, steps
            t += 2 * nu * (int)L.cheb_c1.size() + 3;
        else
            t += 2 + 2 * nu;
    }
    return t;
}

int amg_rz_partials(const AmgState *S) {
    if (!S || S->lv.size() < 2) return 0;
    const AmgLevel &L = S->lv[0];
    if (L.smoother == DPCG_AMG_GAUSS_SEIDEL) return 0;     // (its last pass covers one colour: PCG sums <r, z> itself)
    const int rpb = kBlock / L.tpr_a;
    return (int)std::max<int64_t>(1, std::min<int64_t>((L.A.n + rpb - 1) / rpb, kApplyMaxGrid));
}

int64_t amg_nnz(const AmgState *S) {
    if (!S) return 0;
    int64_t t = 0;
    for (const AmgLevel &L : S->lv) t += L.A.nnz + 2 * L.P.nnz;
    return t;
}

namespace dpcg {
namespace {

// what the cycle reads and writes on a level in storage type W (double: the hierarchy's own arrays; float: the fp32 copies)
template <typename W>
struct LevelView;
template <>
struct LevelView<double> {
    const double *a, *p, *pt, *dinv;
    double *b, *xa, *xb, *ra, *rb, *da, *db;
    explicit LevelView(const AmgLevel &L)
        : a(L.A.val), p(L.P.val), pt(L.Pt.val), dinv(L.dinv), b(L.b), xa(L.xa), xb(L.xb), ra(L.ra), rb(L.rb), da(L.da), db(L.db) {}
};
template <>
struct LevelView<float> {
    const float *a, *p, *pt, *dinv;
    float *b, *xa, *xb, *ra, *rb, *da, *db;
    explicit LevelView(const AmgLevel &L)
        : a(L.a32), p(L.p32), pt(L.pt32), dinv(L.dinv32), b(L.b32), xa(L.xa32), xb(L.xb32), ra(L.ra32), rb(L.rb32), da(L.da32),
          db(L.db32) {}
};

// Down on one level: pre-smoothing, residual, restriction into bnext.  B: the level's right-hand side (level 0: PCG's r, double).
// x / alt: where the level's iterate is and the spare buffer, for the way up.
template <typename W, typename BT>
void level_down(const AmgLevel &L, int nu, const BT *B, W *bnext, W *&x, W *&alt, hipStream_t s, const int *done) {
    const LevelView<W> V(L);
    const W *const nw = nullptr;
    W *const nwo = nullptr;
    if (L.smoother == DPCG_AMG_GAUSS_SEIDEL) {
        if constexpr (std::is_same<W, double>::value) {       // (the fp32 cycle is refused for Gauss-Seidel)
            gs_sweeps(L, nu, true, B, V.xa, s, done);
            launch_row<OP_RES>(L.A, V.a, L.tpr_a, nw, 0.0, B, (const W *)V.xa, nw, nw, nwo, V.ra, nullptr, nullptr, s, done);
            launch_row<OP_PLAIN>(L.Pt, V.pt, L.tpr_pt, nw, 0.0, nw, nw, nw, (const W *)V.ra, bnext, nwo, nullptr, nullptr, s, done);
            x = V.xa;
            alt = V.xb;
        }
        return;
    }
    if (L.smoother == DPCG_AMG_CHEBYSHEV) {       // from x = 0, r = b
        const W *xin = nullptr, *din = nullptr, *rin = nullptr;
        W *xo = V.xa, *xo2 = V.xb, *dn = V.da, *dn2 = V.db, *rn = V.ra, *rn2 = V.rb;
        const int deg = (int)L.cheb_c1.size();
        for (int t = 0; t < nu * deg; ++t) {
            const int k = t % deg;
            const W *dk = k == 0 ? nullptr : din;
            if (t == 0)                           // (r = b, in b's own storage)
                launch_cheb<CHEB_STEP>(L, V.a, V.dinv, L.cheb_c1[k], L.cheb_c2[k], B, xin, dk, B, xo, dn, rn, nullptr, nullptr, s, done);
            else
                launch_cheb<CHEB_STEP>(L, V.a, V.dinv, L.cheb_c1[k], L.cheb_c2[k], B, xin, dk, rin, xo, dn, rn, nullptr, nullptr, s, done);
            xin = xo; din = dn; rin = rn;
            std::swap(xo, xo2); std::swap(dn, dn2); std::swap(rn, rn2);
        }
        launch_row<OP_PLAIN>(L.Pt, V.pt, L.tpr_pt, nw, 0.0, nw, nw, nw, rin, bnext, nwo, nullptr, nullptr, s, done);
        x = const_cast<W *>(xin);
        alt = xo;
        return;
    }
    W *xc = V.xa, *xo = V.xb, *rc = V.ra, *ro = V.rb;
    launch_row<OP_PRE>(L.A, V.a, L.tpr_a, V.dinv, L.omega, B, nw, nw, nw, xc, rc, nullptr, nullptr, s, done);
    for (int k = 1; k < nu; ++k) {
        launch_row<OP_SWEEP>(L.A, V.a, L.tpr_a, V.dinv, L.omega, B, (const W *)xc, (const W *)rc, nw, xo, ro, nullptr, nullptr, s, done);
        std::swap(xc, xo);
        std::swap(rc, ro);
    }
    launch_row<OP_PLAIN>(L.Pt, V.pt, L.tpr_pt, nw, 0.0, nw, nw, nw, (const W *)rc, bnext, nwo, nullptr, nullptr, s, done);
    x = xc;
    alt = xo;
}

// Up on one level: prolongation with correction, post-smoothing.  TOP (level 0): the right-hand side is PCG's r (double) and the last
// smoothing pass writes z to zout, in double, with the <r, z> partials; otherwise it writes a work vector.  Returns where the
// level's result is (null: in zout).
template <typename W, bool TOP>
const W *level_up(const AmgLevel &L, int nu, const std::conditional_t<TOP, double, W> *B, const W *xcoarse, W *x, W *alt, double *zout,
                  double *part_rz, int *n_part_rz, hipStream_t s, const int *done) {
    const LevelView<W> V(L);
    const W *const nw = nullptr;
    W *const nwo = nullptr;
    if (L.smoother == DPCG_AMG_GAUSS_SEIDEL) {    // (level 0 sweeps in z itself)
        if constexpr (std::is_same<W, double>::value) {
            double *out = TOP ? zout : alt;
            launch_row<OP_ACC>(L.P, V.p, L.tpr_p, nw, 0.0, nw, (const W *)x, nw, xcoarse, out, nwo, nullptr, nullptr, s, done);
            gs_sweeps(L, nu, false, B, out, s, done);
            return out;
        }
        return nullptr;
    }
    if (L.smoother == DPCG_AMG_CHEBYSHEV) {
        W *xc = alt, *xo = x, *dn = V.da, *dn2 = V.db, *rn = V.rb, *rn2 = V.ra;
        launch_row<OP_ACC>(L.P, V.p, L.tpr_p, nw, 0.0, nw, (const W *)x, nw, xcoarse, xc, nwo, nullptr, nullptr, s, done);
        launch_row<OP_RES>(L.A, V.a, L.tpr_a, nw, 0.0, B, (const W *)xc, nw, nw, nwo, V.ra, nullptr, nullptr, s, done);
        const W *din = nullptr, *rin = V.ra;
        const int deg = (int)L.cheb_c1.size();
        for (int t = 0; t < nu * deg; ++t) {
            const int k = t % deg;
            const W *dk = k == 0 ? nullptr : din;
            if (t == nu * deg - 1) {
                int grid = 0;
                if constexpr (TOP) {
                    launch_cheb<CHEB_LAST>(L, V.a, V.dinv, L.cheb_c1[k], L.cheb_c2[k], B, (const W *)xc, dk, rin, zout, nwo, nwo, part_rz,
                                           &grid, s, done);
                    if (part_rz && n_part_rz) *n_part_rz = grid;
                    return nullptr;
                } else {
                    launch_cheb<CHEB_LAST>(L, V.a, V.dinv, L.cheb_c1[k], L.cheb_c2[k], B, (const W *)xc, dk, rin, xo, nwo, nwo, nullptr,
                                           &grid, s, done);
                    return xo;
                }
            }
            launch_cheb<CHEB_STEP>(L, V.a, V.dinv, L.cheb_c1[k], L.cheb_c2[k], B, (const W *)xc, dk, rin, xo, dn, rn, nullptr, nullptr, s,
                                   done);
            din = dn; rin = rn;
            std::swap(xc, xo); std::swap(dn, dn2); std::swap(rn, rn2);
        }
        return xc;
    }
    W *xc = x, *xo = alt;
    launch_row<OP_ACC>(L.P, V.p, L.tpr_p, nw, 0.0, nw, (const W *)xc, nw, xcoarse, xo, nwo, nullptr, nullptr, s, done);
    std::swap(xc, xo);
    for (int k = 0; k < nu; ++k) {
        int grid = 0;
        if constexpr (TOP) {
            if (k == nu - 1) {
                launch_row<OP_POST>(L.A, V.a, L.tpr_a, V.dinv, L.omega, B, (const W *)xc, nw, nw, zout, nwo, part_rz, &grid, s, done);
                if (part_rz && n_part_rz) *n_part_rz = grid;
                return nullptr;
            }
        }
        launch_row<OP_POST>(L.A, V.a, L.tpr_a, V.dinv, L.omega, B, (const W *)xc, nw, nw, xo, nwo, nullptr, &grid, s, done);
        std::swap(xc, xo);
    }
    return xc;
}

// one V(nu, nu) cycle with work vectors and operand copies of storage type W
template <typename W>
int apply_cycle(AmgState &S, const double *r, double *z, hipStream_t s, double *part_rz, int *n_part_rz, const int *done) {
    const int Lc = (int)S.lv.size() - 1;
    const int nu = S.sweeps;
    std::vector<W *> x(Lc), alt(Lc);
    for (int l = 0; l < Lc; ++l) {                    // down: pre-smoothing, residual, restriction
        W *bnext = LevelView<W>(S.lv[l + 1]).b;
        if (l == 0) level_down<W, double>(S.lv[l], nu, r, bnext, x[l], alt[l], s, done);
        else level_down<W, W>(S.lv[l], nu, LevelView<W>(S.lv[l]).b, bnext, x[l], alt[l], s, done);
    }
    const LevelView<W> C(S.lv[Lc]);
    hipLaunchKernelGGL(k_amg_gemv<W>, dim3(grid_blocks(S.nco * 64, kAmgGrid)), dim3(kBlock), 0, s, S.nco, S.cinv, (const W *)C.b, C.xa, done);
    const W *xcoarse = C.xa;
    for (int l = Lc - 1; l >= 0; --l) {               // up: prolongation with correction, post-smoothing
        if (l == 0) xcoarse = level_up<W, true>(S.lv[l], nu, r, xcoarse, x[l], alt[l], z, part_rz, n_part_rz, s, done);
        else xcoarse = level_up<W, false>(S.lv[l], nu, LevelView<W>(S.lv[l]).b, xcoarse, x[l], alt[l], nullptr, nullptr, nullptr, s, done);
    }
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

// z = M r by one V(nu, nu) cycle; r, z in the handle's numbering (distinct buffers).  part_rz: the last post-smoothing pass of
// level 0 leaves its per-workgroup partials of <r, z> there (*n_part_rz of them).  done (may be null): the solve's `done` word --
// every kernel returns at once once it is set.
int amg_apply(dpcg_system *h, const double *r, double *z, hipStream_t s, double *part_rz, int *n_part_rz, const int *done) {
    AmgState &S = *h->amg;
    if (n_part_rz) *n_part_rz = 0;
    if (S.lv.size() == 1) {                           // (one level: the dense inverse alone, fp64 in either precision)
        hipLaunchKernelGGL(k_amg_gemv<double>, dim3(grid_blocks(S.nco * 64, kAmgGrid)), dim3(kBlock), 0, s, S.nco, S.cinv, r, z, done);
        return DPCG_OK;
    }
    if (S.precision == DPCG_AMG_FP32) return apply_cycle<float>(S, r, z, s, part_rz, n_part_rz, done);
    return apply_cycle<double>(S, r, z, s, part_rz, n_part_rz, done);
}

extern "C" int dpcg_set_precond_amg(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                                    dpcg_stream_t stream) {
    return dpcg_set_precond_amg_smoothed(h, theta, max_levels, max_coarse, sweeps, seed, DPCG_AMG_JACOBI, 2, 30.0, stream);
}

extern "C" int dpcg_set_precond_amg_smoothed(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                                             int smoother, int degree, double eig_ratio, dpcg_stream_t stream) {
    return dpcg_set_precond_amg_precision(h, theta, max_levels, max_coarse, sweeps, seed, smoother, degree, eig_ratio, DPCG_AMG_FP64,
                                          stream);
}

extern "C" int dpcg_set_precond_amg_precision(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                                              int smoother, int degree, double eig_ratio, int precision, dpcg_stream_t stream) {
    if (!h) return invalid("NULL handle");
    if (!(theta >= 0.0 && theta <= 1.0)) return invalid("dpcg_set_precond_amg: theta must lie in [0, 1]");
    if (max_levels < 1 || max_levels > 64) return invalid("dpcg_set_precond_amg: max_levels must lie in 1 .. 64");
    if (max_coarse < 1) return invalid("dpcg_set_precond_amg: max_coarse must be >= 1");
    if (sweeps < 1 || sweeps > 8) return invalid("dpcg_set_precond_amg: sweeps must lie in 1 .. 8");
    if (smoother != DPCG_AMG_JACOBI && smoother != DPCG_AMG_GAUSS_SEIDEL && smoother != DPCG_AMG_CHEBYSHEV)
        return invalid("dpcg_set_precond_amg_smoothed: unknown smoother (DPCG_AMG_JACOBI, _GAUSS_SEIDEL or _CHEBYSHEV)");
    if (degree < 1 || degree > 8) return invalid("dpcg_set_precond_amg_smoothed: degree must lie in 1 .. 8");
    if (!(eig_ratio > 1.0) || !std::isfinite(eig_ratio)) return invalid("dpcg_set_precond_amg_smoothed: eig_ratio must be finite and > 1");
    if (precision != DPCG_AMG_FP64 && precision != DPCG_AMG_FP32)
        return invalid("dpcg_set_precond_amg_precision: unknown precision (DPCG_AMG_FP64 or DPCG_AMG_FP32)");
    if (precision == DPCG_AMG_FP32 && smoother == DPCG_AMG_GAUSS_SEIDEL)
        return invalid("dpcg_set_precond_amg_precision: the fp32 cycle takes DPCG_AMG_JACOBI and DPCG_AMG_CHEBYSHEV only (Gauss-Seidel's "
                       "cost is its colour passes, not its bytes)");
    if (h->ns)
        return invalid("dpcg_set_precond_amg: the handle has a null space attached (a singular system): the hierarchy's exact coarse solve "
                       "would invert a singular matrix");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);
    AmgState *old = h->amg_parked;
    h->amg_parked = nullptr;
    const bool reusable = old && old->theta == theta && old->max_levels == max_levels &&
                          old->max_coarse == max_coarse && old->seed == seed && old->smoother == smoother && old->degree == degree &&
                          old->eig_ratio == eig_ratio && !old->lv.empty() && old->lv[0].A.n == h->A.n;
    AmgState *S = new AmgState();
    S->theta = theta;
    S->max_levels = max_levels;
    S->max_coarse = max_coarse;
    S->sweeps = sweeps;
    S->seed = seed;
    S->smoother = smoother;
    S->degree = degree;
    S->eig_ratio = eig_ratio;
    S->precision = precision;       // (not among the conditions of `reusable`: copies and work vectors are made anew by every build)
    // built before the attached preconditioner is freed: on failure that one stays (the build reads only the handle's matrix,
    // permutation and cached colouring, none of which belongs to the preconditioner)
    int st = build(h, *S, reusable ? old : nullptr, s);
    free_amg(old);
    if (st >= 0) st = ensure_work(h, 0, false, false);
    if (st < 0) {
        (void)hipStreamSynchronize(s);
        free_amg(S);
        return st;
    }
    free_precond(h);
    h->amg = S;
    h->precond = DPCG_PRECOND_AMG;
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_info(dpcg_handle_t h, int capacity, int *n_levels, int64_t *rows, int64_t *nnz, int64_t *p_nnz,
                                 double *rho, double *omega, double *operator_complexity, double *grid_complexity,
                                 int *reused_levels) {
    if (!h) return invalid("NULL handle");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_info: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    const AmgState &S = *h->amg;
    const int nl = (int)S.lv.size();
    if (n_levels) *n_levels = nl;
    if (reused_levels) *reused_levels = S.reused_levels;
    double sn = 0, sz = 0;
    for (int l = 0; l < nl; ++l) {
        const AmgLevel &L = S.lv[l];
        sn += (double)L.A.n;
        sz += (double)L.A.nnz;
        if (l < capacity) {
            if (rows) rows[l] = L.A.n;
            if (nnz) nnz[l] = L.A.nnz;
            if (p_nnz) p_nnz[l] = L.P.nnz;
            if (rho) rho[l] = L.rho;
            if (omega) omega[l] = L.omega;
        }
    }
    if (operator_complexity) *operator_complexity = sz / (double)S.lv[0].A.nnz;
    if (grid_complexity) *grid_complexity = sn / (double)S.lv[0].A.n;
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_level(dpcg_handle_t h, int level, const int64_t sizes[4], int32_t *agg, int32_t *p_rowptr, int32_t *p_col,
                                  double *p_val, int32_t *a_rowptr, int32_t *a_col, double *a_val, dpcg_stream_t stream) {
    if (!h || !sizes) return invalid("dpcg_get_amg_level: NULL handle or sizes");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_level: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    const AmgState &S = *h->amg;
    if (level < 0 || level >= (int)S.lv.size() - 1) return invalid("dpcg_get_amg_level: level must lie in 0 .. levels - 2");
    const AmgLevel &L = S.lv[level];
    const AmgLevel &N = S.lv[level + 1];
    const int64_t n = L.A.n;
    if (sizes[0] != n || sizes[1] != L.P.nnz || sizes[2] != N.A.n || sizes[3] != N.A.nnz)
        return invalid("dpcg_get_amg_level: the buffers were sized for another hierarchy (ask dpcg_get_amg_info again)");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> perm, a, rp, ci;
    std::vector<double> v;
    if (level == 0 && h->perm) {
        perm.resize(n);
        DPCG_HIP(hipMemcpyAsync(perm.data(), h->perm, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (agg) {
        a.resize(n);
        DPCG_HIP(hipMemcpyAsync(a.data(), L.agg, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    const bool want_p = p_rowptr || p_col || p_val;
    if (want_p) {
        rp.resize(n + 1);
        ci.resize(L.P.nnz);
        v.resize(L.P.nnz);
        DPCG_HIP(hipMemcpyAsync(rp.data(), L.P.rowptr, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipMemcpyAsync(ci.data(), L.P.col, L.P.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipMemcpyAsync(v.data(), L.P.val, L.P.nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (a_rowptr) DPCG_HIP(hipMemcpyAsync(a_rowptr, N.A.rowptr, (N.A.n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (a_col) DPCG_HIP(hipMemcpyAsync(a_col, N.A.col, N.A.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (a_val) DPCG_HIP(hipMemcpyAsync(a_val, N.A.val, N.A.nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    if (agg)
        for (int64_t i = 0; i < n; ++i) agg[perm.empty() ? i : perm[i]] = a[i];     // caller numbering at level 0
    if (want_p) {                                     // rows of P_0 in the caller's numbering
        std::vector<int32_t> orp(n + 1, 0);
        std::vector<int64_t> src(n);                  // caller row -> handle row
        for (int64_t i = 0; i < n; ++i) src[perm.empty() ? i : perm[i]] = i;
        for (int64_t c = 0; c < n; ++c) orp[c + 1] = orp[c] + (rp[src[c] + 1] - rp[src[c]]);
        if (p_rowptr) std::copy(orp.begin(), orp.end(), p_rowptr);
        for (int64_t c = 0; c < n; ++c) {
            const int64_t i = src[c];
            for (int k = rp[i], o = orp[c]; k < rp[i + 1]; ++k, ++o) {
                if (p_col) p_col[o] = ci[k];
                if (p_val) p_val[o] = v[k];
            }
        }
    }
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_precision(dpcg_handle_t h, int *precision) {
    if (!h) return invalid("NULL handle");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_precision: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    if (precision) *precision = h->amg->precision;
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_launches(dpcg_handle_t h, int *launches, int *rz_partials) {
    if (!h) return invalid("NULL handle");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_launches: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    if (launches) *launches = amg_launches(h->amg);
    if (rz_partials) *rz_partials = amg_rz_partials(h->amg);
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_smoothers(dpcg_handle_t h, int capacity, int *smoother, int *n_colors, double *cheb_lower, double *cheb_upper) {
    if (!h) return invalid("NULL handle");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_smoothers: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    const AmgState &S = *h->amg;
    for (int l = 0; l + 1 < (int)S.lv.size() && l < capacity; ++l) {
        const AmgLevel &L = S.lv[l];
        const bool gs = L.smoother == DPCG_AMG_GAUSS_SEIDEL, ch = L.smoother == DPCG_AMG_CHEBYSHEV;
        if (smoother) smoother[l] = L.smoother;
        if (n_colors) n_colors[l] = gs ? (int)L.gs_off.size() - 1 : 0;
        if (cheb_lower) cheb_lower[l] = ch ? L.cheb_lo : 0.0;
        if (cheb_upper) cheb_upper[l] = ch ? L.cheb_hi : 0.0;
    }
    return DPCG_OK;
}

extern "C" int dpcg_get_amg_colors(dpcg_handle_t h, int level, int64_t n, int32_t *color, dpcg_stream_t stream) {
    if (!h) return invalid("NULL handle");
    if (h->precond != DPCG_PRECOND_AMG || !h->amg) {
        set_error("dpcg_get_amg_colors: no smoothed-aggregation preconditioner is attached");
        return DPCG_ERR_STATE;
    }
    const AmgState &S = *h->amg;
    if (level < 0 || level >= (int)S.lv.size() - 1) return invalid("dpcg_get_amg_colors: level must lie in 0 .. levels - 2");
    const AmgLevel &L = S.lv[level];
    if (L.smoother != DPCG_AMG_GAUSS_SEIDEL) {
        set_error("dpcg_get_amg_colors: the level is not smoothed by Gauss-Seidel");
        return DPCG_ERR_STATE;
    }
    if (n != L.A.n || !color) return invalid("dpcg_get_amg_colors: n is not the level's number of rows (or color is NULL)");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> rows(n), perm;
    DPCG_HIP(hipMemcpyAsync(rows.data(), L.gs_rows, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (level == 0 && h->perm) {
        perm.resize(n);
        DPCG_HIP(hipMemcpyAsync(perm.data(), h->perm, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    DPCG_HIP(hipStreamSynchronize(s));
    for (int c = 0; c + 1 < (int)L.gs_off.size(); ++c)
        for (int32_t p = L.gs_off[c]; p < L.gs_off[c + 1]; ++p) color[perm.empty() ? rows[p] : perm[rows[p]]] = c;
    return DPCG_OK;
}
