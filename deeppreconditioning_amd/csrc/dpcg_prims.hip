// The building blocks of the setup routines (see dpcg_prims.h): rocPRIM-backed device-wide primitives -- this is the one translation
// unit that instantiates rocPRIM templates, so the rest of the library compiles in seconds -- the generic index kernels, and the CSR
// transpose built from both.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

#include "dpcg_host.h"

namespace dpcg {

namespace {
struct Scratch {
    void *p = nullptr;
    ~Scratch() {
        if (p) cached_free(p);
    }
    int reserve(size_t bytes) {
        if (cached_alloc(&p, bytes ? bytes : 1) != hipSuccess) {
            p = nullptr;
            set_error("device primitive: scratch allocation failed");
            return DPCG_ERR_NOMEM;
        }
        return DPCG_OK;
    }
};

#define PRIM_HIP(call)                                                   \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

template <typename K>
int sort_pairs(const K *keys_in, K *keys_out, const int32_t *vals_in, int32_t *vals_out, int64_t count, int end_bit,
               hipStream_t s) {
    if (count <= 0) return DPCG_OK;
    if (end_bit < 1) end_bit = 1;
    if (end_bit > (int)(8 * sizeof(K))) end_bit = (int)(8 * sizeof(K));
    size_t bytes = 0;
    PRIM_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)count, 0u,
                                       (unsigned)end_bit, s));
    Scratch tmp;
    if (int st = tmp.reserve(bytes); st < 0) return st;
    PRIM_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)count, 0u,
                                       (unsigned)end_bit, s));
    PRIM_HIP(hipStreamSynchronize(s));   // the scratch buffer is released on return
    return DPCG_OK;
}
}  // namespace

int sort_pairs_u64_i32(const uint64_t *keys_in, uint64_t *keys_out, const int32_t *vals_in, int32_t *vals_out,
                       int64_t count, int end_bit, hipStream_t s) {
    return sort_pairs<uint64_t>(keys_in, keys_out, vals_in, vals_out, count, end_bit, s);
}

int sort_pairs_u32_i32(const uint32_t *keys_in, uint32_t *keys_out, const int32_t *vals_in, int32_t *vals_out,
                       int64_t count, int end_bit, hipStream_t s) {
    return sort_pairs<uint32_t>(keys_in, keys_out, vals_in, vals_out, count, end_bit, s);
}

int exclusive_scan_i32(const int32_t *in, int32_t *out, int64_t count, hipStream_t s) {
    if (count <= 0) return DPCG_OK;
    size_t bytes = 0;
    PRIM_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, (int32_t)0, (size_t)count, rocprim::plus<int32_t>(), s));
    Scratch tmp;
    if (int st = tmp.reserve(bytes); st < 0) return st;
    PRIM_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, (int32_t)0, (size_t)count, rocprim::plus<int32_t>(), s));
    PRIM_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// The same scan with the caller's workspace (scan_workspace_bytes(count) bytes): no allocation, no synchronisation.
size_t scan_workspace_bytes(int64_t count) {
    size_t bytes = 0;
    if (count <= 0) return 0;
    if (rocprim::exclusive_scan(nullptr, bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)count,
                                rocprim::plus<int32_t>(), nullptr) != hipSuccess)
        return 0;
    return bytes;
}

int exclusive_scan_i32_ws(const int32_t *in, int32_t *out, int64_t count, void *workspace, size_t workspace_bytes, hipStream_t s) {
    if (count <= 0) return DPCG_OK;
    size_t bytes = workspace_bytes;
    PRIM_HIP(rocprim::exclusive_scan(workspace, bytes, in, out, (int32_t)0, (size_t)count, rocprim::plus<int32_t>(), s));
    return DPCG_OK;
}

int inclusive_scan_i32(const int32_t *in, int32_t *out, int64_t count, hipStream_t s) {
    if (count <= 0) return DPCG_OK;
    size_t bytes = 0;
    PRIM_HIP(rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)count, rocprim::plus<int32_t>(), s));
    Scratch tmp;
    if (int st = tmp.reserve(bytes); st < 0) return st;
    PRIM_HIP(rocprim::inclusive_scan(tmp.p, bytes, in, out, (size_t)count, rocprim::plus<int32_t>(), s));
    PRIM_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

int reduce_max_i32(const int32_t *in, int32_t *out_dev, int64_t count, hipStream_t s) {
    if (count <= 0) return DPCG_OK;
    size_t bytes = 0;
    PRIM_HIP(rocprim::reduce(nullptr, bytes, in, out_dev, (int32_t)(-2147483647 - 1), (size_t)count,
                             rocprim::maximum<int32_t>(), s));
    Scratch tmp;
    if (int st = tmp.reserve(bytes); st < 0) return st;
    PRIM_HIP(rocprim::reduce(tmp.p, bytes, in, out_dev, (int32_t)(-2147483647 - 1), (size_t)count,
                             rocprim::maximum<int32_t>(), s));
    PRIM_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// ---- index kernels -----------------------------------------------------------------------------------------------------------
namespace {
constexpr int kIndexGrid = 8192;      // most workgroups of an index kernel ...
constexpr int kVectorGrid = 2048;     // ... and of a gather / scatter of a vector (these run in a reordered handle's solves too)
}  // namespace

__global__ __launch_bounds__(kBlock) void k_row_of(int64_t n, const int32_t *__restrict__ rp, int32_t *__restrict__ row_of) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        for (int k = rp[i]; k < rp[i + 1]; ++k) row_of[k] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_iota(int64_t count, int32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += stride) out[k] = (int32_t)k;
}

// Offsets of the groups of a SORTED key array: ptr[g] = first position with key >= g, for g = 0..groups (ptr[groups] =
// count).  Empty groups get the offset of the next non-empty one.
__global__ __launch_bounds__(kBlock) void k_group_offsets(int64_t count, const uint32_t *__restrict__ keys, int groups,
                                                          int32_t *__restrict__ ptr) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= count; k += stride) {
        const int64_t lo = k == 0 ? 0 : (int64_t)keys[k - 1] + 1;
        const int64_t hi = k == count ? groups : (int64_t)keys[k];
        for (int64_t g = lo; g <= hi; ++g) ptr[g] = (int32_t)k;
    }
}

// Entries of the transposed matrix from the sort permutation: tcol[d] = row_of[perm[d]], tval[d] = val[perm[d]].
__global__ __launch_bounds__(kBlock) void k_transpose_gather(int64_t nnz, const int32_t *__restrict__ perm,
                                                             const int32_t *__restrict__ row_of,
                                                             const double *__restrict__ val, int32_t *__restrict__ tcol,
                                                             double *__restrict__ tval) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t d = (int64_t)blockIdx.x * kBlock + threadIdx.x; d < nnz; d += stride) {
        const int32_t k = perm[d];
        tcol[d] = row_of[k];
        tval[d] = val[k];
    }
}

__global__ __launch_bounds__(kBlock) void k_invert_positions(int64_t n, const int32_t *__restrict__ rows, int32_t *__restrict__ pos) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) pos[rows[j]] = (int32_t)j;
}

__global__ __launch_bounds__(kBlock) void k_compose_positions(int64_t n, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ pos, int32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) out[j] = pos[rows[j]];
}

namespace {
__global__ __launch_bounds__(kBlock) void k_relabel(int64_t count, const int32_t *__restrict__ map, int32_t *__restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += stride) idx[k] = map[idx[k]];
}

__global__ __launch_bounds__(kBlock) void k_same_i32(int64_t count, const int32_t *__restrict__ a, const int32_t *__restrict__ b, int *differ) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    bool d = false;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < count; k += stride) d |= a[k] != b[k];
    if (d) *differ = 1;      // (every writer stores the same value)
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_gather_vec(int64_t n, const int32_t *__restrict__ perm, const T *__restrict__ in,
                                                       T *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) out[r] = in[perm[r]];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_scatter_vec(int64_t n, const int32_t *__restrict__ perm, const T *__restrict__ in,
                                                        T *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) out[perm[r]] = in[r];
}
}  // namespace

void launch_row_of(int64_t n, const int32_t *rp, int32_t *row_of, hipStream_t s) {
    hipLaunchKernelGGL(k_row_of, dim3(grid_blocks(n, kIndexGrid)), dim3(kBlock), 0, s, n, rp, row_of);
}
void launch_iota(int64_t count, int32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_iota, dim3(grid_blocks(count, kIndexGrid)), dim3(kBlock), 0, s, count, out);
}
void launch_group_offsets(int64_t count, const uint32_t *keys_sorted, int groups, int32_t *ptr, hipStream_t s) {
    hipLaunchKernelGGL(k_group_offsets, dim3(grid_blocks(count + 1, kIndexGrid)), dim3(kBlock), 0, s, count, keys_sorted, groups, ptr);
}
void launch_transpose_gather(int64_t nnz, const int32_t *perm, const int32_t *row_of, const double *val, int32_t *tcol,
                             double *tval, hipStream_t s) {
    hipLaunchKernelGGL(k_transpose_gather, dim3(grid_blocks(nnz, kIndexGrid)), dim3(kBlock), 0, s, nnz, perm, row_of, val, tcol, tval);
}
void launch_invert_positions(int64_t n, const int32_t *rows, int32_t *pos, hipStream_t s) {
    hipLaunchKernelGGL(k_invert_positions, dim3(grid_blocks(n, kIndexGrid)), dim3(kBlock), 0, s, n, rows, pos);
}
void launch_compose_positions(int64_t n, const int32_t *rows, const int32_t *pos, int32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(k_compose_positions, dim3(grid_blocks(n, kIndexGrid)), dim3(kBlock), 0, s, n, rows, pos, out);
}
void launch_relabel(int64_t count, const int32_t *map, int32_t *idx, hipStream_t s) {
    hipLaunchKernelGGL(k_relabel, dim3(grid_blocks(count, kIndexGrid)), dim3(kBlock), 0, s, count, map, idx);
}
void launch_same_i32(int64_t count, const int32_t *a, const int32_t *b, int *differ_flag, hipStream_t s) {
    hipLaunchKernelGGL(k_same_i32, dim3(grid_blocks(count, 65535)), dim3(kBlock), 0, s, count, a, b, differ_flag);
}
void launch_gather_f64(int64_t n, const int32_t *perm, const double *in, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_vec<double>, dim3(grid_blocks(n, kVectorGrid)), dim3(kBlock), 0, s, n, perm, in, out);
}
void launch_scatter_f64(int64_t n, const int32_t *perm, const double *in, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_scatter_vec<double>, dim3(grid_blocks(n, kVectorGrid)), dim3(kBlock), 0, s, n, perm, in, out);
}
void launch_gather_f32(int64_t n, const int32_t *perm, const float *in, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_vec<float>, dim3(grid_blocks(n, kVectorGrid)), dim3(kBlock), 0, s, n, perm, in, out);
}
void launch_scatter_f32(int64_t n, const int32_t *perm, const float *in, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_scatter_vec<float>, dim3(grid_blocks(n, kVectorGrid)), dim3(kBlock), 0, s, n, perm, in, out);
}

// ---- the CSR transpose (see dpcg_prims.h) ------------------------------------------------------------------------------------
int transpose_csr(int64_t rows, int64_t cols, int64_t nnz, const int32_t *rp, const int32_t *ci, const double *val,
                  int32_t *out_rp, int32_t *out_ci, double *out_val, int32_t *order, hipStream_t s) {
    DevBuf<int32_t> row_of, iota;
    DevBuf<uint32_t> cols_sorted;
    DPCG_TRY(row_of.alloc(nnz));
    DPCG_TRY(iota.alloc(nnz));
    DPCG_TRY(cols_sorted.alloc(nnz));
    launch_row_of(rows, rp, row_of.p, s);
    launch_iota(nnz, iota.p, s);
    DPCG_TRY(sort_pairs_u32_i32(reinterpret_cast<const uint32_t *>(ci), cols_sorted.p, iota.p, order, nnz,
                                bits_for((uint64_t)std::max<int64_t>(1, cols - 1)), s));
    launch_group_offsets(nnz, cols_sorted.p, (int)cols, out_rp, s);
    if (val) launch_transpose_gather(nnz, order, row_of.p, val, out_ci, out_val, s);
    else launch_compose_positions(nnz, order, row_of.p, out_ci, s);          // out_ci[d] = row_of[order[d]]
    return DPCG_OK;
}

}  // namespace dpcg
