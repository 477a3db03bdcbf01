// Plan-side pieces shared by the two sparse-convolution forwards (dpcg_convnet.hip: PreconditionerNet, dpcg_unet.hip:
// PreconditionerSparseUNet): the slab allocator of a plan, the input sites as CSR over the image rows, and the
// lower-triangular CSR (col <= row) of the output sites that the factor L is written into.
#pragma once

#include <utility>
#include <vector>

#include "dpcg_host.h"

namespace dpcg {
namespace {

// Hands out the plan's arrays from its slabs in a fixed order: a rebuild draws from them again (a slab grows only when the
// new pattern needs more), so a stream of similar matrices -- one plan per matrix -- costs no device allocations after the
// first.  P has `std::vector<std::pair<void *, size_t>> slabs` and `size_t slab_cursor`.
template <typename P, typename T>
int plan_alloc(P *p, T **out, int64_t count) {
    const size_t bytes = (size_t)(count < 1 ? 1 : count) * sizeof(T);
    *out = nullptr;
    if (p->slab_cursor < p->slabs.size()) {
        auto &sl = p->slabs[p->slab_cursor];
        if (sl.second < bytes) {
            (void)device_free(sl.first);
            sl = {nullptr, 0};
            const size_t grown = bytes + bytes / 4;
            if (hipMalloc(&sl.first, grown) != hipSuccess) {
                set_error("dpcg sparse-conv plan: device allocation failed");
                return DPCG_ERR_NOMEM;
            }
            sl.second = grown;
        }
        *out = reinterpret_cast<T *>(sl.first);
        ++p->slab_cursor;
        return DPCG_OK;
    }
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) {
        set_error("dpcg sparse-conv plan: device allocation failed");
        return DPCG_ERR_NOMEM;
    }
    p->slabs.emplace_back(q, bytes);
    ++p->slab_cursor;
    *out = reinterpret_cast<T *>(q);
    return DPCG_OK;
}

constexpr int kConvGrid = 4096;       // most workgroups of a kernel of the sparse-convolution forward passes

// Input sites (nnz, 3) = (batch, row, col), sorted by (batch, row, col): row pointers over batch * H rows, the column
// array, and a check of the order.  Thread i owns site i and fills the row pointers of the rows that START at or before
// it and after the previous site's row (empty rows in between included).
__global__ __launch_bounds__(kBlock) void k_sites_to_csr(int64_t nnz, const int32_t *__restrict__ idx, int batch, int64_t H,
                                                         int64_t W, int32_t *__restrict__ rowptr, int32_t *__restrict__ col,
                                                         int *bad) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t rows = (int64_t)batch * H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += stride) {
        const int b = idx[3 * i], y = idx[3 * i + 1], x = idx[3 * i + 2];
        if (b < 0 || b >= batch || y < 0 || y >= H || x < 0 || x >= W) {
            atomicExch(bad, 1);
            continue;
        }
        const int64_t r = (int64_t)b * H + y;
        int64_t rprev = -1;
        if (i > 0) {
            const int pb = idx[3 * i - 3], py = idx[3 * i - 2], px = idx[3 * i - 1];
            rprev = (int64_t)pb * H + py;
            if (rprev > r || (rprev == r && px >= x)) atomicExch(bad, 2);      // not sorted / duplicate site
        }
        col[i] = x;
        for (int64_t rr = rprev + 1; rr <= r; ++rr) rowptr[rr] = (int32_t)i;
        if (i == nnz - 1)
            for (int64_t rr = r + 1; rr <= rows; ++rr) rowptr[rr] = (int32_t)nnz;
    }
}

// rows of the sites, and the lower-triangular part (col <= row: a prefix of every sorted row)
__global__ __launch_bounds__(kBlock) void k_lower_count(int64_t rows, int64_t H, const int32_t *__restrict__ rp,
                                                        const int32_t *__restrict__ col, int32_t *__restrict__ len,
                                                        int32_t *__restrict__ site_row, int32_t *__restrict__ site_batch) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= rows; r += stride) {
        if (r == rows) {
            len[r] = 0;
            continue;
        }
        const int y = (int)(r % H), b = (int)(r / H);
        int c = 0;
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            site_row[k] = y;
            site_batch[k] = b;
            c += col[k] <= y ? 1 : 0;
        }
        len[r] = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_lower_fill(int64_t rows, int64_t H, const int32_t *__restrict__ rp,
                                                       const int32_t *__restrict__ col, const int32_t *__restrict__ lrp,
                                                       int32_t *__restrict__ lcol, int32_t *__restrict__ lpos) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
        const int y = (int)(r % H);
        int at = lrp[r];
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            if (col[k] <= y) {
                lcol[at] = col[k];
                lpos[k] = at++;
            } else {
                lpos[k] = -1;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_out_indices(int64_t sites, const int32_t *__restrict__ site_batch,
                                                        const int32_t *__restrict__ site_row, const int32_t *__restrict__ col,
                                                        int32_t *__restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sites; i += stride) {
        idx[3 * i] = site_batch[i];
        idx[3 * i + 1] = site_row[i];
        idx[3 * i + 2] = col[i];
    }
}

}  // namespace
}  // namespace dpcg
