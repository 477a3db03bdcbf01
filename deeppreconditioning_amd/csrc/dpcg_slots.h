// Several sums at once, for the vector kernels that carry a small block of columns through PCG (dpcg_nullspace.hip, dpcg_deflation.hip):
// N running sums per lane -> wave tree -> four wave sums each in LDS -> one fixed-order add, and the per-workgroup partials of such
// sums kept in "slots" of kMaxGrid doubles that every workgroup of a later kernel re-reduces in the same order.  Include from .hip
// files only.
#pragma once

#include "dpcg_device.h"

namespace dpcg {

template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double *sh) {   // sh: 4 N doubles
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int j = 0; j < N; ++j) sh[4 * j + (threadIdx.x >> 6)] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = ((sh[4 * j] + sh[4 * j + 1]) + sh[4 * j + 2]) + sh[4 * j + 3];
}

// slots first .. first + N - 1 of the partial buffer, G partials each, summed as reduce_partials sums them
template <int N>
__device__ __forceinline__ void reduce_slots(const double *__restrict__ part, int first, int G, double (&v)[N], double *sh) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double *__restrict__ pj = part + (int64_t)(first + j) * kMaxGrid;
        double s = 0.0;
        for (int i = threadIdx.x; i < G; i += kBlock) s += pj[i];
        v[j] = s;
    }
    block_sum_n<N>(v, sh);
}

template <int N>
__device__ __forceinline__ void store_slots(double *__restrict__ part, int first, const double (&v)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) part[(int64_t)(first + j) * kMaxGrid + blockIdx.x] = v[j];
}

}  // namespace dpcg
