// ILU(0) and DILU: the zero-fill L U factorisations behind dpcg_set_precond_ilu0 (contract: tests/ilu0_restatement.py).  The
// pattern of A (rows sorted) is split into L (strict lower part, then a unit diagonal stored last) and U (the diagonal first, then
// the strict upper part); the values are those of A until the numeric phase has been over them.
//
// Row i depends only on the finished rows k < i of its own lower pattern -- the dependency graph of the lower solve -- so the
// numeric phase runs level by level on the level sets of L's pattern (compute_levels), one launch per level, one lane per row
// (rows are short: a stencil's).  In multicolour order that is about as many launches as there are colours.
//   ILU(0)  for the stored k < i ascending: l_ik = a_ik / u_kk, then for the stored (k, j), j > k ascending, a_ij -= l_ik u_kj where
//           (i, j) is stored -- both rows ascend, so row i is searched by two cursors that only move forward (one in its L
//           part, one in its U part).  Every entry receives its subtractions in ascending k.
//   DILU    OpenFOAM's rule: d_i = a_ii - sum over the stored k < i ascending, (k, i) stored too, of (a_ik a_ki) / d_k; l_ik = a_ik / d_k;
//           U keeps A's strict upper part.  A missing (k, i) contributes nothing.
// One product, one division, one subtraction at a time (-ffp-contract=off): the factor equals the restatement bit for bit.
// A pivot that is zero or not finite is reported as 0x7fffffff - row through an atomic maximum: the FIRST such row wins, the rows
// that then divide by it do not hide it.
#include "dpcg_host.h"
#include "dpcg_prims.h"

namespace dpcg {
namespace {

constexpr int kIlu0Grid = 8192;       // most workgroups of the two pattern kernels (they stride over the rows)

// cl[i] = entries of row i left of the diagonal + 1 (the unit diagonal), cu[i] = entries at or right of it; cl[n] = cu[n] = 0 for the
// scans; *flag = 1 when a row stores no diagonal
__global__ __launch_bounds__(kBlock) void k_ilu0_count(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       int32_t *__restrict__ cl, int32_t *__restrict__ cu, int *flag) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) {
        if (i == n) {
            cl[i] = 0;
            cu[i] = 0;
            continue;
        }
        int lower = 0, diag = 0;
        const int e = rp[i + 1];
        for (int k = rp[i]; k < e; ++k) {
            const int c = ci[k];
            lower += c < i ? 1 : 0;
            diag |= c == i ? 1 : 0;
        }
        cl[i] = lower + 1;
        cu[i] = (e - rp[i]) - lower;
        if (!diag) atomicExch(flag, 1);
    }
}

// (columns ascend: the L part of a row is its first cl[i] - 1 entries, the U part the rest, the diagonal leading it)
__global__ __launch_bounds__(kBlock) void k_ilu0_split(int64_t n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                       const double *__restrict__ v, const int32_t *__restrict__ lrp,
                                                       int32_t *__restrict__ lci, double *__restrict__ lv,
                                                       const int32_t *__restrict__ urp, int32_t *__restrict__ uci,
                                                       double *__restrict__ uv) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int src = rp[i], la = lrp[i], nl = lrp[i + 1] - la - 1, ua = urp[i], nu = urp[i + 1] - ua;
        for (int q = 0; q < nl; ++q) {
            lci[la + q] = ci[src + q];
            lv[la + q] = v[src + q];
        }
        lci[la + nl] = (int32_t)i;
        lv[la + nl] = 1.0;
        for (int q = 0; q < nu; ++q) {
            uci[ua + q] = ci[src + nl + q];
            uv[ua + q] = v[src + nl + q];
        }
    }
}

// One level of the numeric phase: row rows[j0 + idx] of L and U in place.  The rows k it reads belong to earlier levels (launches).
template <bool DILU>
__global__ __launch_bounds__(kBlock) void k_ilu0_level(const int32_t *__restrict__ rows, int j0, int count,
                                                       const int32_t *__restrict__ lrp, const int32_t *__restrict__ lci, double *lv,
                                                       const int32_t *__restrict__ urp, const int32_t *__restrict__ uci, double *uv,
                                                       int *bad) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= count) return;
    const int i = rows[j0 + idx];
    const int ls = lrp[i], le = lrp[i + 1] - 1;           // (the unit diagonal stays out)
    const int us = urp[i], ue = urp[i + 1];
    double d = uv[us];
    for (int a = ls; a < le; ++a) {
        const int k = lci[a];
        const int ks = urp[k], ke = urp[k + 1];
        const double pivot = uv[ks];
        if (DILU) {
            const double aik = lv[a];
            for (int b = ks + 1; b < ke; ++b) {
                const int j = uci[b];
                if (j < i) continue;
                if (j == i) {
                    double t = aik * uv[b];
                    t = t / pivot;
                    d = d - t;
                }
                break;
            }
            lv[a] = aik / pivot;
        } else {
            const double l = lv[a] / pivot;
            lv[a] = l;
            int pa = a + 1, pb = us;
            for (int b = ks + 1; b < ke; ++b) {
                const int j = uci[b];
                const double p = l * uv[b];
                if (j < i) {
                    while (pa < le && lci[pa] < j) ++pa;
                    if (pa < le && lci[pa] == j) lv[pa] = lv[pa] - p;
                } else {
                    while (pb < ue && uci[pb] < j) ++pb;
                    if (pb < ue && uci[pb] == j) uv[pb] = uv[pb] - p;
                }
            }
        }
    }
    if (DILU) uv[us] = d;
    else d = uv[us];
    if (d == 0.0 || !isfinite(d)) atomicMax(bad, 0x7fffffff - i);
}

}  // namespace

void launch_ilu0_count(int64_t n, const int32_t *rp, const int32_t *ci, int32_t *cl, int32_t *cu, int *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_ilu0_count, dim3(grid_blocks(n + 1, kIlu0Grid)), dim3(kBlock), 0, s, n, rp, ci, cl, cu, flag);
}

void launch_ilu0_split(int64_t n, const int32_t *rp, const int32_t *ci, const double *v, const int32_t *lrp, int32_t *lci, double *lv,
                       const int32_t *urp, int32_t *uci, double *uv, hipStream_t s) {
    hipLaunchKernelGGL(k_ilu0_split, dim3(grid_blocks(n, kIlu0Grid)), dim3(kBlock), 0, s, n, rp, ci, v, lrp, lci, lv, urp, uci, uv);
}

void launch_ilu0_level(bool dilu, const int32_t *rows, int j0, int count, const int32_t *lrp, const int32_t *lci, double *lv,
                       const int32_t *urp, const int32_t *uci, double *uv, int *bad, hipStream_t s) {
    const dim3 grid((unsigned)grid_blocks(count, 0x7fffffff));
    if (dilu) hipLaunchKernelGGL(k_ilu0_level<true>, grid, dim3(kBlock), 0, s, rows, j0, count, lrp, lci, lv, urp, uci, uv, bad);
    else hipLaunchKernelGGL(k_ilu0_level<false>, grid, dim3(kBlock), 0, s, rows, j0, count, lrp, lci, lv, urp, uci, uv, bad);
}

}  // namespace dpcg
