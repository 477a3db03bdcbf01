// Building blocks of the setup routines (COO -> CSR, transpose, level sets, reordering, every preconditioner setup), compiled once in
// dpcg_prims.hip:
//   * device-wide sort / scan / reduce: thin, non-template entry points over rocPRIM; every call allocates its own scratch;
//   * the generic index kernels (iota, row of an entry, group offsets, inverse and composed maps, relabel, gather / scatter);
//   * transpose_csr, the CSR transpose every factor and prolongation goes through.
// Setup paths only -- nothing here runs inside the PCG iteration except the gathers / scatters of a reordered handle's vectors.
// The routines that can fail return a dpcg_status.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpcg {

// Stable LSD radix sort of (key, value) pairs on bits [0, end_bit) of the key.  in/out must not alias.
int sort_pairs_u64_i32(const uint64_t *keys_in, uint64_t *keys_out, const int32_t *vals_in, int32_t *vals_out,
                       int64_t count, int end_bit, hipStream_t s);
int sort_pairs_u32_i32(const uint32_t *keys_in, uint32_t *keys_out, const int32_t *vals_in, int32_t *vals_out,
                       int64_t count, int end_bit, hipStream_t s);
// out[i] = in[0] + ... + in[i-1] (exclusive) or ... + in[i] (inclusive); in == out is allowed.
int exclusive_scan_i32(const int32_t *in, int32_t *out, int64_t count, hipStream_t s);
int inclusive_scan_i32(const int32_t *in, int32_t *out, int64_t count, hipStream_t s);
// exclusive scan in a caller-provided workspace of scan_workspace_bytes(count) bytes: no allocation, no synchronisation
size_t scan_workspace_bytes(int64_t count);
int exclusive_scan_i32_ws(const int32_t *in, int32_t *out, int64_t count, void *workspace, size_t workspace_bytes, hipStream_t s);
// *out_dev = max(in[0..count))
int reduce_max_i32(const int32_t *in, int32_t *out_dev, int64_t count, hipStream_t s);
// number of bits needed to represent values in [0, max_value]
inline int bits_for(uint64_t max_value) {
    int b = 1;
    while (b < 64 && (max_value >> b) != 0) ++b;
    return b;
}

// ---- index kernels -----------------------------------------------------------------------------------------------------------
void launch_iota(int64_t count, int32_t *out, hipStream_t s);                                           // out[k] = k
void launch_row_of(int64_t n, const int32_t *rp, int32_t *row_of, hipStream_t s);                       // row_of[k] = the row of entry k
// ptr[g] = first position with key >= g in a SORTED key array, g = 0 .. groups (ptr[groups] = count)
void launch_group_offsets(int64_t count, const uint32_t *keys_sorted, int groups, int32_t *ptr, hipStream_t s);
// tcol[d] = row_of[perm[d]], tval[d] = val[perm[d]]
void launch_transpose_gather(int64_t nnz, const int32_t *perm, const int32_t *row_of, const double *val, int32_t *tcol,
                             double *tval, hipStream_t s);
void launch_invert_positions(int64_t n, const int32_t *rows, int32_t *pos, hipStream_t s);          // pos[rows[j]] = j
void launch_compose_positions(int64_t n, const int32_t *rows, const int32_t *pos, int32_t *out, hipStream_t s);   // out[j] = pos[rows[j]]
void launch_relabel(int64_t count, const int32_t *map, int32_t *idx, hipStream_t s);                    // idx[k] = map[idx[k]]
void launch_same_i32(int64_t count, const int32_t *a, const int32_t *b, int *differ_flag, hipStream_t s);   // *differ_flag = 1 where a[k] != b[k]
void launch_gather_f64(int64_t n, const int32_t *perm, const double *in, double *out, hipStream_t s);    // out[r] = in[perm[r]]
void launch_scatter_f64(int64_t n, const int32_t *perm, const double *in, double *out, hipStream_t s);   // out[perm[r]] = in[r]
void launch_gather_f32(int64_t n, const int32_t *perm, const float *in, float *out, hipStream_t s);
void launch_scatter_f32(int64_t n, const int32_t *perm, const float *in, float *out, hipStream_t s);

// B = A^T as CSR by a stable sort of A's entries by column: the rows of A ascend inside every row of B (for a lower factor with
// the diagonal last, B has it first).  A: rows x cols, nnz entries.  order[d] = the entry of A that entry d of B is (always written).
// out_val / val may both be null: pattern only.  Enqueues on s, does not synchronise.  Its temporaries are freed on return, while
// the last kernels may still read them: a freed block is reused only by the same SetupScope on the same stream, and outside a
// scope a free waits for the device (dpcg_mem.hip).
int transpose_csr(int64_t rows, int64_t cols, int64_t nnz, const int32_t *rp, const int32_t *ci, const double *val,
                  int32_t *out_rp, int32_t *out_ci, double *out_val, int32_t *order, hipStream_t s);

}  // namespace dpcg
