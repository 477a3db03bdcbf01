// Block-Jacobi incomplete Cholesky (DPCG_PRECOND_BLOCK_LLT_SOLVE, include/dpcg.h; contract: tests/block_ic_restatement.py): the
// unknowns are partitioned into blocks of at most 4096 rows, couplings between blocks are dropped, every block is factored on its
// own (IC(0) or DIC) and solved by ONE workgroup with the block's slice of the vector in LDS -- no workgroup waits for another, one
// launch applies the whole preconditioner.
//
// Factor numbering: rows sorted stably by (block id, caller's row); perm_c[k] = the caller's row at factor position k.  A block is a
// run [blk_ptr[b], blk_ptr[b + 1]) of positions; L = the factor of A_B (P A P^T without the entries that cross blocks) as one CSR in
// that numbering (dpcg_get_factor).  What the kernels read is a second copy per triangular factor (BicSide): a block's rows listed
// level by level, its off-diagonal entries stored in the order the levels visit them with 16-bit block-local columns, the diagonal
// by level-order position.  Setup runs on the device: the sort (dpcg_prims.h), the extraction of tril(A_B) and of its transpose
// (a stable sort of the entries by column), the level sets (one workgroup per block, k_bic_levels) and the values (k_bic_ic0 /
// k_bic_dic, one workgroup per block walking the levels of L).  Everything that depends on the pattern and the block ids only stays
// on the handle across dpcg_update_values; the next attach with the same ids computes only values.
#include <climits>
#include <cstring>
#include <memory>

#include "dpcg_host.h"
#include "dpcg_prims.h"

namespace dpcg {
constexpr int kBicMaxRows = 4096;      // rows of a block: its slice of the vector is one LDS array of doubles (32 KiB)
constexpr int kBicSetupThreads = 256;  // workgroup of the setup kernels (levels, values)
constexpr int kBicGrid = 4096;         // most workgroups of a setup kernel that strides over rows

struct BicSide {                       // one triangular factor as the solve kernel reads it
    int32_t *nlev = nullptr;           // [nblocks] levels of a block
    int32_t *lvl_ptr = nullptr;        // [n + nblocks] block b's level offsets (block-local positions, nlev + 1 of them) at blk_ptr[b] + b
    uint16_t *row = nullptr;           // [n] block-local row at level-order position
    int32_t *e_ptr = nullptr;          // [n + 1] off-diagonal entries of the row at a position (the rows of a level: one contiguous run)
    uint16_t *e_col = nullptr;         // [nnz - n] block-local column
    int32_t *e_src = nullptr;          // [nnz - n] the entry of L it is
    int32_t *d_src = nullptr;          // [n] the entry of L the diagonal at a position is
    double *e_val = nullptr, *diag = nullptr;
    int max_levels = 0;
};

struct BlockIc {
    int64_t n = 0, nnz = 0;
    int variant = 0, nblocks = 0, max_block = 0, threads = 0;
    bool attached = false, reused = false;
    int32_t *ids = nullptr;            // [n] the caller's block ids (what a later attach is compared with)
    int32_t *perm_c = nullptr;         // [n] factor position -> caller's row
    int32_t *hperm = nullptr;          // [n] factor position -> handle index (perm_c itself unless the handle is reordered)
    int32_t *blk_ptr = nullptr;        // [nblocks + 1]
    int32_t *rp = nullptr, *ci = nullptr, *map_al = nullptr;   // L's pattern (factor numbering) and entry of L -> entry of the caller's matrix
    double *val = nullptr;             // L's values
    BicSide lo, up;
};
}  // namespace dpcg

namespace {
void free_side(BicSide &s) {
    dev_free(s.nlev); dev_free(s.lvl_ptr); dev_free(s.row); dev_free(s.e_ptr); dev_free(s.e_col); dev_free(s.e_src); dev_free(s.d_src);
    dev_free(s.e_val); dev_free(s.diag);
}

// ---- symbolic phase ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bic_contiguous_ids(int64_t n, int block_rows, int32_t *__restrict__ ids) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) ids[i] = (int32_t)(i / block_rows);
}

// flags[0] = the first row with a negative id (INT_MAX: none)
__global__ __launch_bounds__(kBlock) void k_bic_check_ids(int64_t n, const int32_t *__restrict__ ids, int *flags) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        if (ids[i] < 0) atomicMin(flags, (int)i);
}

// head[k] = 1 where a new block begins at sorted position k > 0 (the inclusive scan of it is the block's index)
__global__ __launch_bounds__(kBlock) void k_bic_block_heads(int64_t n, const uint32_t *__restrict__ keys_sorted, int32_t *__restrict__ head) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride)
        head[k] = (k > 0 && keys_sorted[k] != keys_sorted[k - 1]) ? 1 : 0;
}

// out[0] = the largest block, out[1] = the first block of more than kBicMaxRows rows (INT_MAX: none)
__global__ __launch_bounds__(kBlock) void k_bic_block_sizes(int nblocks, const int32_t *__restrict__ blk_ptr, int *out) {
    const int stride = gridDim.x * kBlock;
    for (int b = blockIdx.x * kBlock + threadIdx.x; b < nblocks; b += stride) {
        const int m = blk_ptr[b + 1] - blk_ptr[b];
        atomicMax(out, m);
        if (m > kBicMaxRows) atomicMin(out + 1, b);
    }
}

// Row k of tril(A_B) = the entries (i, j) of the caller's row i = perm_c[k] with id[j] == id[i] and j <= i (inside a block the factor
// order is the caller's, so ascending j is ascending factor position).  WRITE = false: counts them and checks the row -- flags[0] the
// first caller's row whose columns do not strictly ascend, flags[1] the first one without a diagonal (INT_MAX: none).
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void k_bic_tril(int64_t n, const int32_t *__restrict__ perm_c, const int32_t *__restrict__ pos,
                                                     const int32_t *__restrict__ ids, const int32_t *__restrict__ arp,
                                                     const int32_t *__restrict__ aci, int32_t *__restrict__ cnt, const int32_t *__restrict__ lrp,
                                                     int32_t *__restrict__ lci, int32_t *__restrict__ map_al, int *flags) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const int i = perm_c[k], id = ids[i];
        int c = 0, prev = -1;
        bool diag = false, sorted = true;
        int o = WRITE ? lrp[k] : 0;
        for (int e = arp[i]; e < arp[i + 1]; ++e) {
            const int j = aci[e];
            if (!WRITE) {
                sorted = sorted && j > prev;
                prev = j;
                diag = diag || j == i;
            }
            if (j < 0 || j >= n || j > i || ids[j] != id) continue;
            if (WRITE) {
                lci[o] = pos[j];
                map_al[o] = e;
                ++o;
            } else {
                ++c;
            }
        }
        if (!WRITE) {
            cnt[k] = c;
            if (!sorted) atomicMin(flags, i);
            if (!diag) atomicMin(flags + 1, i);
        }
    }
}

// The level sets of one block of a triangular factor and its level-ordered copy: one workgroup per block.  Round t gives level t to
// the rows whose dependencies all got their level in an earlier round; rows of a level are listed in ascending order.  stats[0] /
// stats[1]: most levels of a block (L / L^T), stats[2]: a round that placed no row (cannot happen on a triangular pattern).
template <bool UPPER>
__global__ __launch_bounds__(kBicSetupThreads) void k_bic_levels(int n, const int32_t *__restrict__ blk_ptr, const int32_t *__restrict__ rp,
                                                                 const int32_t *__restrict__ ci, const int32_t *__restrict__ src,
                                                                 int32_t *__restrict__ nlev_out, int32_t *__restrict__ lvl_ptr,
                                                                 uint16_t *__restrict__ row_out, int32_t *__restrict__ e_ptr,
                                                                 uint16_t *__restrict__ e_col, int32_t *__restrict__ e_src,
                                                                 int32_t *__restrict__ d_src, int *stats) {
    __shared__ int lev[kBicMaxRows];
    __shared__ int cnt[kBicMaxRows];           // rows per level, then the cursor of a level, then the entry offset of a position
    __shared__ uint16_t len[kBicMaxRows];
    __shared__ uint16_t ord[kBicMaxRows];
    __shared__ int s_new;
    const int b = blockIdx.x, tid = threadIdx.x, r0 = blk_ptr[b], m = blk_ptr[b + 1] - r0;
    for (int i = tid; i < m; i += kBicSetupThreads) {
        lev[i] = -1;
        cnt[i] = 0;
        len[i] = (uint16_t)(rp[r0 + i + 1] - rp[r0 + i] - 1);
    }
    __syncthreads();
    int total = 0, t = 0;
    for (;; ++t) {
        if (tid == 0) s_new = 0;
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < m; i += kBicSetupThreads) {
            if (lev[i] >= 0) continue;
            const int s = rp[r0 + i] + (UPPER ? 1 : 0), e = rp[r0 + i + 1] - (UPPER ? 0 : 1);
            bool ready = true;
            for (int k = s; k < e && ready; ++k) {
                const int lj = lev[ci[k] - r0];          // (a level written in this very round reads as t: not ready)
                ready = lj >= 0 && lj < t;
            }
            if (ready) {
                lev[i] = t;
                ++mine;
            }
        }
        if (mine) atomicAdd(&s_new, mine);
        __syncthreads();
        const int placed = s_new;
        total += placed;
        __syncthreads();
        if (total >= m || placed == 0) break;
    }
    if (total < m) {
        if (tid == 0) atomicExch(stats + 2, 1);
        return;
    }
    const int nlev = t + 1;
    for (int i = tid; i < m; i += kBicSetupThreads) atomicAdd(&cnt[lev[i]], 1);
    __syncthreads();
    if (tid == 0) {
        int32_t *lp = lvl_ptr + r0 + b;
        int acc = 0;
        for (int l = 0; l < nlev; ++l) {
            const int c = cnt[l];
            lp[l] = acc;
            cnt[l] = acc;
            acc += c;
        }
        lp[nlev] = acc;
        for (int i = 0; i < m; ++i) ord[cnt[lev[i]]++] = (uint16_t)i;
        int eo = rp[r0] - r0;                             // off-diagonal entries ahead of this block (every row has one diagonal)
        for (int p = 0; p < m; ++p) {
            cnt[p] = eo;
            eo += len[ord[p]];
        }
        nlev_out[b] = nlev;
        atomicMax(stats + (UPPER ? 1 : 0), nlev);
        if (r0 + m == n) e_ptr[n] = eo;
    }
    __syncthreads();
    for (int p = tid; p < m; p += kBicSetupThreads) {
        const int i = ord[p];
        row_out[r0 + p] = (uint16_t)i;
        e_ptr[r0 + p] = cnt[p];
        const int s = rp[r0 + i] + (UPPER ? 1 : 0), e = rp[r0 + i + 1] - (UPPER ? 0 : 1);
        const int dk = UPPER ? rp[r0 + i] : rp[r0 + i + 1] - 1;
        d_src[r0 + p] = src ? src[dk] : dk;
        int o = cnt[p];
        for (int k = s; k < e; ++k, ++o) {
            e_col[o] = (uint16_t)(ci[k] - r0);
            e_src[o] = src ? src[k] : k;
        }
    }
}

// ---- values ----------------------------------------------------------------------------------------------------------------------
// IC(0) of a block, level by level (one workgroup per block, a row per lane): the loop of k_ic0_level (dpcg_sptrsv.hip) -- sums over
// ascending columns, one product and one subtraction at a time -- so the factor equals oracle.ic0(A_B) bit for bit.  val holds
// tril(A_B) on entry and L on exit.  bad: the first factor position with a non-positive or non-finite pivot (INT_MAX: none).
__global__ __launch_bounds__(kBicSetupThreads) void k_bic_ic0(const int32_t *__restrict__ blk_ptr, const int32_t *__restrict__ nlev,
                                                              const int32_t *__restrict__ lvl_ptr, const uint16_t *__restrict__ row,
                                                              const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, double *val, int *bad) {
    const int b = blockIdx.x, r0 = blk_ptr[b];
    const int32_t *lp = lvl_ptr + r0 + b;
    const int nl = nlev[b];
    for (int l = 0; l < nl; ++l) {
        for (int p = lp[l] + threadIdx.x; p < lp[l + 1]; p += kBicSetupThreads) {
            const int i = r0 + row[r0 + p];
            const int s_i = rp[i], e_i = rp[i + 1];
            for (int k = s_i; k < e_i; ++k) {
                const int j = ci[k];
                const int s_j = rp[j], e_j = rp[j + 1];
                double acc = val[k];
                int a = s_i, c = s_j;
                while (a < k && c < e_j - 1) {
                    const int ca = ci[a], cb = ci[c];
                    if (ca == cb) {
                        acc -= val[a] * val[c];
                        ++a;
                        ++c;
                    } else if (ca < cb) ++a;
                    else ++c;
                }
                if (j < i) {
                    val[k] = acc / val[e_j - 1];
                } else {
                    if (!(acc > 0.0) || !isfinite(acc)) atomicMin(bad, i);
                    val[k] = sqrt(acc);
                }
            }
        }
        __syncthreads();
    }
}

// DIC of a block: d_i = a_ii - sum_j (a_ij a_ij) / d_j over the stored j < i ascending (one product, one division, one subtraction per
// term), level by level with d in LDS; then L_ij = a_ij / sqrt(d_j), L_ii = sqrt(d_i).
__global__ __launch_bounds__(kBicSetupThreads) void k_bic_dic(const int32_t *__restrict__ blk_ptr, const int32_t *__restrict__ nlev,
                                                              const int32_t *__restrict__ lvl_ptr, const uint16_t *__restrict__ row,
                                                              const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, double *val, int *bad) {
    __shared__ double d[kBicMaxRows];
    const int b = blockIdx.x, r0 = blk_ptr[b], m = blk_ptr[b + 1] - r0;
    const int32_t *lp = lvl_ptr + r0 + b;
    const int nl = nlev[b];
    for (int l = 0; l < nl; ++l) {
        for (int p = lp[l] + threadIdx.x; p < lp[l + 1]; p += kBicSetupThreads) {
            const int li = row[r0 + p], i = r0 + li;
            const int e = rp[i + 1] - 1;
            double acc = val[e];
            for (int k = rp[i]; k < e; ++k) {
                const double a = val[k];
                double t = a * a;
                t = t / d[ci[k] - r0];
                acc = acc - t;
            }
            if (!(acc > 0.0) || !isfinite(acc)) atomicMin(bad, i);
            d[li] = acc;
        }
        __syncthreads();
    }
    for (int li = threadIdx.x; li < m; li += kBicSetupThreads) d[li] = sqrt(d[li]);
    __syncthreads();
    for (int li = threadIdx.x; li < m; li += kBicSetupThreads) {
        const int i = r0 + li, e = rp[i + 1] - 1;
        for (int k = rp[i]; k < e; ++k) val[k] = val[k] / d[ci[k] - r0];
        val[e] = d[li];
    }
}

// ---- the apply ---------------------------------------------------------------------------------------------------------------------
struct BicApply {
    const int32_t *blk_ptr, *hperm;
    const int32_t *lo_nlev, *lo_lvl, *lo_eptr, *up_nlev, *up_lvl, *up_eptr;
    const uint16_t *lo_row, *lo_col, *up_row, *up_col;
    const double *lo_val, *lo_diag, *up_val, *up_diag;
    const double *r;
    double *z, *part_rz;
    const int *done;
    int max_block;
};

// One triangular solve of a block in place in LDS: level by level, a row per lane, the row's sum in CSR order and then the division
// (oracle.sptrsv_lower / sptrsv_upper_t); a barrier of the workgroup between levels.  lp: the block's level offsets (LDS).
template <int T>
__device__ __forceinline__ void bic_solve_side(double *x, const uint16_t *lp, int nl, int m, int r0, const uint16_t *__restrict__ row,
                                               const int32_t *__restrict__ eptr, const uint16_t *__restrict__ col, const double *__restrict__ val,
                                               const double *__restrict__ diag) {
    for (int l = 0; l < nl; ++l) {
        const int p1 = l + 1 < nl ? (int)lp[l + 1] : m;
        for (int p = (int)lp[l] + (int)threadIdx.x; p < p1; p += T) {
            const int i = row[r0 + p];
            const int k1 = eptr[r0 + p + 1];
            double acc = x[i];
            for (int k = eptr[r0 + p]; k < k1; ++k) acc = acc - val[k] * x[col[k]];
            x[i] = acc / diag[r0 + p];
        }
        __syncthreads();
    }
}

// z = P^T L^-T L^-1 P r, one workgroup per block: the block's slice of r gathered through hperm into LDS, L solved in place, then L^T,
// z scattered through hperm.  With part_rz the workgroup also leaves its share of <r, z>: a lane's terms in ascending order, the lanes
// by a fixed halving tree.  LDS: max_block doubles (x), T doubles (the tree), 2 x max_block 16-bit level offsets.
template <int T>
__global__ __launch_bounds__(T) void k_block_ic_solve(BicApply a) {
    extern __shared__ double bic_lds[];
    if (a.done && *a.done) return;
    double *x = bic_lds;
    double *red = x + a.max_block;
    uint16_t *lpl = reinterpret_cast<uint16_t *>(red + T);
    uint16_t *lpu = lpl + a.max_block;
    const int b = blockIdx.x, tid = threadIdx.x, r0 = a.blk_ptr[b], m = a.blk_ptr[b + 1] - r0;
    const int nl = a.lo_nlev[b], nu = a.up_nlev[b];
    for (int i = tid; i < m; i += T) x[i] = a.r[a.hperm[r0 + i]];
    for (int l = tid; l < nl; l += T) lpl[l] = (uint16_t)a.lo_lvl[r0 + b + l];
    for (int l = tid; l < nu; l += T) lpu[l] = (uint16_t)a.up_lvl[r0 + b + l];
    __syncthreads();
    bic_solve_side<T>(x, lpl, nl, m, r0, a.lo_row, a.lo_eptr, a.lo_col, a.lo_val, a.lo_diag);
    bic_solve_side<T>(x, lpu, nu, m, r0, a.up_row, a.up_eptr, a.up_col, a.up_val, a.up_diag);
    double acc = 0.0;
    for (int i = tid; i < m; i += T) {
        const int g = a.hperm[r0 + i];
        const double zi = x[i];
        a.z[g] = zi;
        if (a.part_rz) acc += a.r[g] * zi;
    }
    if (a.part_rz) {
        red[tid] = acc;
        __syncthreads();
        for (int w = T / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.part_rz[b] = red[0];
    }
}

// Workgroup size by the largest block: a block of up to 64 rows is one wave (its barriers cost nothing), and no size gets more lanes
// than its widest levels can use (a box of m rows of a grid has levels of ~m^(2/3) rows).  DPCG_BLOCK_IC_THREADS: development knob.
int bic_threads(int max_block) {
    static const int knob = [] { const char *e = getenv("DPCG_BLOCK_IC_THREADS"); return e ? atoi(e) : 0; }();
    if (knob == 64 || knob == 128 || knob == 256 || knob == 512 || knob == 1024) return knob;
    return max_block <= 64 ? 64 : (max_block <= 512 ? 128 : (max_block <= 2048 ? 256 : 512));
}

size_t bic_lds_bytes(int max_block, int threads) {
    return (size_t)max_block * sizeof(double) + (size_t)threads * sizeof(double) + 2 * (size_t)max_block * sizeof(uint16_t);
}

void free_bic(BlockIc *c) {
    if (!c) return;
    dev_free(c->ids); dev_free(c->perm_c); dev_free(c->hperm); dev_free(c->blk_ptr); dev_free(c->rp); dev_free(c->ci); dev_free(c->map_al);
    dev_free(c->val);
    free_side(c->lo);
    free_side(c->up);
    delete c;
}

int alloc_side(BicSide &s, int64_t n, int64_t nnz, int nblocks) {
    DPCG_TRY(dev_alloc(&s.nlev, nblocks));
    DPCG_TRY(dev_alloc(&s.lvl_ptr, n + nblocks));
    DPCG_TRY(dev_alloc(&s.row, n));
    DPCG_TRY(dev_alloc(&s.e_ptr, n + 1));
    DPCG_TRY(dev_alloc(&s.e_col, nnz - n));
    DPCG_TRY(dev_alloc(&s.e_src, nnz - n));
    DPCG_TRY(dev_alloc(&s.d_src, n));
    DPCG_TRY(dev_alloc(&s.e_val, nnz - n));
    DPCG_TRY(dev_alloc(&s.diag, n));
    return DPCG_OK;
}

// factor position -> handle index
int bic_handle_map(dpcg_system *h, BlockIc *c, hipStream_t s) {
    if (!c->hperm) DPCG_TRY(dev_alloc(&c->hperm, c->n));
    if (h->iperm) launch_compose_positions(c->n, c->perm_c, h->iperm, c->hperm, s);
    else DPCG_HIP(hipMemcpyAsync(c->hperm, c->perm_c, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return DPCG_OK;
}

// The symbolic phase: numbering, tril(A_B) and its transpose, level sets and level-ordered copies.  ids: on the device, taken over.
int bic_symbolic(dpcg_system *h, const CsrDev &A, int32_t *ids_dev, BlockIc **out, hipStream_t s) {
    const int64_t n = A.n;
    std::unique_ptr<BlockIc, void (*)(BlockIc *)> c(new BlockIc(), free_bic);
    c->n = n;
    c->ids = ids_dev;
    DevBuf<int> flags;
    DevBuf<int32_t> iota, head, pos, cnt;
    DevBuf<uint32_t> keys_sorted;
    DPCG_TRY(flags.alloc(8));
    DPCG_TRY(iota.alloc(n));
    DPCG_TRY(head.alloc(n));
    DPCG_TRY(pos.alloc(n));
    DPCG_TRY(cnt.alloc(n + 1));
    DPCG_TRY(keys_sorted.alloc(n));
    DPCG_TRY(dev_alloc(&c->perm_c, n));
    int h_flags[8];
    for (int q = 0; q < 8; ++q) h_flags[q] = INT_MAX;
    h_flags[2] = 0;                                            // [0] negative id, [1] --, [2] largest block, [3] first oversized block
    DPCG_HIP(hipMemcpyAsync(flags.p, h_flags, sizeof(h_flags), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_bic_check_ids, dim3(grid_blocks(n, kBicGrid)), dim3(kBlock), 0, s, n, c->ids, flags.p);
    DPCG_TRY(fetch(h_flags, flags.p, 1, s));
    if (h_flags[0] != INT_MAX) {
        set_error("block IC: negative block id at row " + std::to_string(h_flags[0]));
        return DPCG_ERR_INVALID;
    }
    // rows sorted stably by block id; blocks = the maximal runs of equal id
    launch_iota(n, iota.p, s);
    DPCG_TRY(sort_pairs_u32_i32(reinterpret_cast<const uint32_t *>(c->ids), keys_sorted.p, iota.p, c->perm_c, n, 31, s));
    hipLaunchKernelGGL(k_bic_block_heads, dim3(grid_blocks(n, kBicGrid)), dim3(kBlock), 0, s, n, keys_sorted.p, head.p);
    DPCG_TRY(inclusive_scan_i32(head.p, head.p, n, s));
    int32_t last = 0;
    DPCG_TRY(fetch(&last, head.p + (n - 1), 1, s));
    c->nblocks = last + 1;
    DPCG_TRY(dev_alloc(&c->blk_ptr, c->nblocks + 1));
    launch_group_offsets(n, reinterpret_cast<const uint32_t *>(head.p), c->nblocks, c->blk_ptr, s);
    hipLaunchKernelGGL(k_bic_block_sizes, dim3(grid_blocks(c->nblocks, kBicGrid)), dim3(kBlock), 0, s, c->nblocks, c->blk_ptr, flags.p + 2);
    DPCG_TRY(fetch(h_flags + 2, flags.p + 2, 2, s));
    c->max_block = h_flags[2];
    if (h_flags[3] != INT_MAX) {
        int32_t bp[2] = {0, 0};
        uint32_t id = 0;
        DPCG_TRY(fetch(bp, c->blk_ptr + h_flags[3], 2, s));
        DPCG_TRY(fetch(&id, keys_sorted.p + bp[0], 1, s));
        set_error("block IC: block id " + std::to_string(id) + " holds " + std::to_string(bp[1] - bp[0]) + " rows (at most " +
                  std::to_string(kBicMaxRows) + ")");
        return DPCG_ERR_INVALID;
    }
    // tril(A_B) in the factor numbering
    launch_invert_positions(n, c->perm_c, pos.p, s);
    h_flags[4] = h_flags[5] = INT_MAX;
    DPCG_HIP(hipMemcpyAsync(flags.p + 4, h_flags + 4, 2 * sizeof(int), hipMemcpyHostToDevice, s));
    DPCG_HIP(hipMemsetAsync(cnt.p + n, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_bic_tril<false>, dim3(grid_blocks(n, kBicGrid)), dim3(kBlock), 0, s, n, c->perm_c, pos.p, c->ids, A.rowptr, A.col, cnt.p,
                       nullptr, nullptr, nullptr, flags.p + 4);
    DPCG_TRY(dev_alloc(&c->rp, n + 1));
    DPCG_TRY(exclusive_scan_i32(cnt.p, c->rp, n + 1, s));
    int32_t lnnz = 0;
    DPCG_HIP(hipMemcpyAsync(h_flags + 4, flags.p + 4, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    DPCG_TRY(fetch(&lnnz, c->rp + n, 1, s));
    if (h_flags[4] != INT_MAX) {
        set_error("block IC: the columns of row " + std::to_string(h_flags[4]) + " are not strictly ascending");
        return DPCG_ERR_INVALID;
    }
    if (h_flags[5] != INT_MAX) {
        set_error("block IC: missing diagonal entry at row " + std::to_string(h_flags[5]));
        return DPCG_ERR_INVALID;
    }
    c->nnz = lnnz;
    DPCG_TRY(dev_alloc(&c->ci, c->nnz));
    DPCG_TRY(dev_alloc(&c->map_al, c->nnz));
    DPCG_TRY(dev_alloc(&c->val, c->nnz));
    hipLaunchKernelGGL(k_bic_tril<true>, dim3(grid_blocks(n, kBicGrid)), dim3(kBlock), 0, s, n, c->perm_c, pos.p, c->ids, A.rowptr, A.col, nullptr,
                       c->rp, c->ci, c->map_al, nullptr);
    // L^T's pattern (the rows of a column come out ascending, the diagonal first)
    DevBuf<int32_t> order, trp, tci;
    DPCG_TRY(order.alloc(c->nnz));
    DPCG_TRY(trp.alloc(n + 1));
    DPCG_TRY(tci.alloc(c->nnz));
    DPCG_TRY(transpose_csr(n, n, c->nnz, c->rp, c->ci, nullptr, trp.p, tci.p, nullptr, order.p, s));
    // level sets and level-ordered copies, block by block
    DPCG_TRY(alloc_side(c->lo, n, c->nnz, c->nblocks));
    DPCG_TRY(alloc_side(c->up, n, c->nnz, c->nblocks));
    DPCG_HIP(hipMemsetAsync(flags.p, 0, 3 * sizeof(int), s));
    hipLaunchKernelGGL(k_bic_levels<false>, dim3(c->nblocks), dim3(kBicSetupThreads), 0, s, (int)n, c->blk_ptr, c->rp, c->ci, nullptr, c->lo.nlev,
                       c->lo.lvl_ptr, c->lo.row, c->lo.e_ptr, c->lo.e_col, c->lo.e_src, c->lo.d_src, flags.p);
    hipLaunchKernelGGL(k_bic_levels<true>, dim3(c->nblocks), dim3(kBicSetupThreads), 0, s, (int)n, c->blk_ptr, trp.p, tci.p, order.p, c->up.nlev,
                       c->up.lvl_ptr, c->up.row, c->up.e_ptr, c->up.e_col, c->up.e_src, c->up.d_src, flags.p);
    DPCG_TRY(fetch(h_flags, flags.p, 3, s));
    DPCG_CHECK_LAUNCH();
    if (h_flags[2]) {
        set_error("block IC: the level analysis of a block did not finish");
        return DPCG_ERR_STATE;
    }
    c->lo.max_levels = h_flags[0];
    c->up.max_levels = h_flags[1];
    c->threads = bic_threads(c->max_block);
    DPCG_TRY(bic_handle_map(h, c.get(), s));
    *out = c.release();
    return DPCG_OK;
}

// The values of the factor from the matrix's current values into `val` (nnz doubles); DPCG_ERR_PIVOT names the caller's row.
int bic_numeric(const BlockIc *c, const CsrDev &A, int variant, double *val, hipStream_t s) {
    DevBuf<int> bad;
    DPCG_TRY(bad.alloc(1));
    int h_bad = INT_MAX;
    DPCG_HIP(hipMemcpyAsync(bad.p, &h_bad, sizeof(int), hipMemcpyHostToDevice, s));
    launch_gather_f64(c->nnz, c->map_al, A.val, val, s);
    if (variant == DPCG_BLOCK_IC_DIC)
        hipLaunchKernelGGL(k_bic_dic, dim3(c->nblocks), dim3(kBicSetupThreads), 0, s, c->blk_ptr, c->lo.nlev, c->lo.lvl_ptr, c->lo.row, c->rp, c->ci, val,
                           bad.p);
    else
        hipLaunchKernelGGL(k_bic_ic0, dim3(c->nblocks), dim3(kBicSetupThreads), 0, s, c->blk_ptr, c->lo.nlev, c->lo.lvl_ptr, c->lo.row, c->rp, c->ci, val,
                           bad.p);
    DPCG_TRY(fetch(&h_bad, bad.p, 1, s));
    DPCG_CHECK_LAUNCH();
    if (h_bad != INT_MAX) {
        int32_t row = 0;
        DPCG_HIP(hipMemcpy(&row, c->perm_c + h_bad, sizeof(int32_t), hipMemcpyDeviceToHost));
        set_error(std::string(variant == DPCG_BLOCK_IC_DIC ? "block DIC" : "block IC(0)") + ": non-positive or non-finite pivot at row " +
                  std::to_string(row));
        return DPCG_ERR_PIVOT;
    }
    return DPCG_OK;
}

void bic_load_values(BlockIc *c, hipStream_t s) {
    const int64_t off = c->nnz - c->n;
    for (BicSide *sd : {&c->lo, &c->up}) {
        launch_gather_f64(off, sd->e_src, c->val, sd->e_val, s);
        launch_gather_f64(c->n, sd->d_src, c->val, sd->diag, s);
    }
}
}  // namespace

void free_block_ic(BlockIc *&c) {
    free_bic(c);
    c = nullptr;
}

void block_ic_detach(BlockIc *c) {
    if (c) c->attached = false;
}

// dpcg_reorder: the factor and its numbering are the caller's, only the way into the handle's vectors changes
int block_ic_renumbered(dpcg_system *h, hipStream_t s) {
    if (!h->bic) return DPCG_OK;
    DPCG_TRY(bic_handle_map(h, h->bic, s));
    DPCG_HIP(hipStreamSynchronize(s));
    h->bic->attached = true;
    h->precond = DPCG_PRECOND_BLOCK_LLT_SOLVE;
    return DPCG_OK;
}

int block_ic_rz_partials(const BlockIc *c) { return c && c->nblocks <= kMaxSpmvGrid ? c->nblocks : 0; }
int64_t block_ic_nnz(const BlockIc *c) { return c ? c->nnz : 0; }

int block_ic_apply(dpcg_system *h, const double *r, double *z, hipStream_t s, double *part_rz, int *n_part_rz, const int *done) {
    const BlockIc *c = h->bic;
    if (!c || !c->attached) {
        set_error("block IC: no factor attached");
        return DPCG_ERR_STATE;
    }
    const bool dot = part_rz && n_part_rz && block_ic_rz_partials(c) > 0;
    BicApply a;
    a.blk_ptr = c->blk_ptr; a.hperm = c->hperm;
    a.lo_nlev = c->lo.nlev; a.lo_lvl = c->lo.lvl_ptr; a.lo_eptr = c->lo.e_ptr; a.lo_row = c->lo.row; a.lo_col = c->lo.e_col;
    a.lo_val = c->lo.e_val; a.lo_diag = c->lo.diag;
    a.up_nlev = c->up.nlev; a.up_lvl = c->up.lvl_ptr; a.up_eptr = c->up.e_ptr; a.up_row = c->up.row; a.up_col = c->up.e_col;
    a.up_val = c->up.e_val; a.up_diag = c->up.diag;
    a.r = r; a.z = z; a.part_rz = dot ? part_rz : nullptr; a.done = done; a.max_block = c->max_block;
    const size_t lds = bic_lds_bytes(c->max_block, c->threads);
    switch (c->threads) {
        case 64: hipLaunchKernelGGL(k_block_ic_solve<64>, dim3(c->nblocks), dim3(64), lds, s, a); break;
        case 128: hipLaunchKernelGGL(k_block_ic_solve<128>, dim3(c->nblocks), dim3(128), lds, s, a); break;
        case 256: hipLaunchKernelGGL(k_block_ic_solve<256>, dim3(c->nblocks), dim3(256), lds, s, a); break;
        case 512: hipLaunchKernelGGL(k_block_ic_solve<512>, dim3(c->nblocks), dim3(512), lds, s, a); break;
        default: hipLaunchKernelGGL(k_block_ic_solve<1024>, dim3(c->nblocks), dim3(1024), lds, s, a); break;
    }
    if (dot) *n_part_rz = c->nblocks;
    return DPCG_OK;
}

extern "C" int dpcg_set_precond_block_ic(dpcg_handle_t h, int variant, int block_rows, const int32_t *block_of_row, int memspace,
                                         dpcg_stream_t stream) {
    if (!h) return invalid("NULL handle");
    if (variant != DPCG_BLOCK_IC_IC0 && variant != DPCG_BLOCK_IC_DIC) return invalid("dpcg_set_precond_block_ic: variant must be IC(0) or DIC");
    if (!block_of_row && (block_rows < 1 || block_rows > kBicMaxRows)) return invalid("dpcg_set_precond_block_ic: block_rows must be in 1 .. 4096");
    if (block_of_row && memspace != DPCG_HOST && memspace != DPCG_DEVICE) return invalid("dpcg_set_precond_block_ic: bad memspace");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);          // (the preconditioner being replaced may be in use on another stream)
    const CsrDev &A = h->perm ? h->A_user : h->A;      // blocks and factor are the caller's: a reordered handle gives the same bits
    const int64_t n = A.n;
    DevBuf<int32_t> ids;
    DPCG_TRY(ids.alloc(n));
    if (block_of_row) {
        const hipError_t e = hipMemcpyAsync(ids.p, block_of_row, (size_t)n * sizeof(int32_t),
                                            memspace == DPCG_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return hip_fail(e != hipSuccess ? e : hipGetLastError(), "block IC: block ids", __FILE__, __LINE__);
    } else {
        hipLaunchKernelGGL(k_bic_contiguous_ids, dim3(grid_blocks(n, kBicGrid)), dim3(kBlock), 0, s, n, block_rows, ids.p);
    }
    // the same ids as the symbolic phase on the handle was built for: only the values are computed
    BlockIc *c = h->bic;
    bool reuse = false;
    if (c && c->n == n) {
        DevBuf<int> differ;
        int h_differ = 1;
        DPCG_TRY(differ.alloc(1));
        DPCG_HIP(hipMemsetAsync(differ.p, 0, sizeof(int), s));
        launch_same_i32(n, ids.p, c->ids, differ.p, s);
        DPCG_TRY(fetch(&h_differ, differ.p, 1, s));
        reuse = h_differ == 0;
    }
    if (!reuse) {
        c = nullptr;
        DPCG_TRY(bic_symbolic(h, A, ids.release(), &c, s));          // (takes ids over, on failure too)
    }
    DevBuf<double> val;
    int st = val.alloc(c->nnz);
    if (st >= 0) st = bic_numeric(c, A, variant, val.p, s);
    if (st < 0) {                                            // the previous preconditioner -- this very factor perhaps -- stays as it was
        if (!reuse) free_bic(c);
        return st;
    }
    if (!reuse && h->bic) free_block_ic(h->bic);
    h->bic = nullptr;
    free_precond(h);                                         // (frees everything else, a parked factor included)
    h->bic = c;
    std::swap(c->val, val.p);
    bic_load_values(c, s);
    st = bic_handle_map(h, c, s);
    if (st >= 0 && (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess)) st = DPCG_ERR_HIP;
    if (st < 0) {
        free_block_ic(h->bic);
        return st;
    }
    c->variant = variant;
    c->reused = reuse;
    c->attached = true;
    h->precond = DPCG_PRECOND_BLOCK_LLT_SOLVE;
    return DPCG_OK;
}

extern "C" int dpcg_get_block_ic_info(dpcg_handle_t h, int32_t out[8]) {
    if (!h || !out) return invalid("dpcg_get_block_ic_info: NULL handle or output");
    const BlockIc *c = h->bic;
    if (h->precond != DPCG_PRECOND_BLOCK_LLT_SOLVE || !c || !c->attached) {
        set_error("dpcg_get_block_ic_info: the attached preconditioner is not a block incomplete-Cholesky factor");
        return DPCG_ERR_STATE;
    }
    out[0] = c->variant;
    out[1] = c->nblocks;
    out[2] = c->max_block;
    out[3] = c->lo.max_levels;
    out[4] = c->up.max_levels;
    out[5] = c->threads;
    out[6] = c->reused ? 1 : 0;
    out[7] = 0;
    return DPCG_OK;
}

int block_ic_get_factor(const dpcg_system *h, int32_t *rowptr, int32_t *col, double *val) {
    const BlockIc *c = h->bic;
    DPCG_HIP(hipMemcpy(rowptr, c->rp, (size_t)(c->n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPCG_HIP(hipMemcpy(col, c->ci, (size_t)c->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    DPCG_HIP(hipMemcpy(val, c->val, (size_t)c->nnz * sizeof(double), hipMemcpyDeviceToHost));
    return DPCG_OK;
}

int block_ic_get_ordering(const dpcg_system *h, int32_t *perm_host) {
    DPCG_HIP(hipMemcpy(perm_host, h->bic->perm_c, (size_t)h->bic->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return DPCG_OK;
}
