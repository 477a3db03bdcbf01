// Singular (symmetric positive SEMI-definite) systems: a null space attached to the handle and projected inside PCG
// (dpcg_set_nullspace / dpcg_get_nullspace, include/dpcg.h).  Not in the reference, whose systems are all definite.
// Compiled with -ffp-contract=off like dpcg_pcg.hip.
//
// Z is n x k with orthonormal columns (1 <= k <= 4), P = I - Z Z^T.  The solve (the contract is in include/dpcg.h):
//     b' = P b;  r = b' - A x0 (x0 given: r = P r once);  zt = M r;  s = Z^T zt;  t = Z^T r;  rho = <r,zt> - t^T s;  p = zt - Z s
//     update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  zt = M r (NOT projected in memory);
//              s = Z^T zt;  t = Z^T r;  rho' = <r,zt> - t^T s;  p = (zt - Z s) + (rho'/rho) p
//     end:     x = x - Z (Z^T x)
// The recurrence's kernels and the launch of an update are dpcg_projected.h's, over NullBasis (U = V = Z; rho = <r,zt> - t^T s).
// CONST: Z = 1/sqrt(n), one column, never read -- K2 and K3 then move exactly the bytes of k_update_r / k_update_xp (40 per row
// each with Jacobi); a general Z adds 8k bytes per row to each pass.  Here: the projections of b, r and x, the check of A Z = 0, the
// attach and the solve.
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_projected.h"

namespace dpcg {

constexpr int kNsMaxK = 4;
// partial slots (dpcg_projected.h): <r,r>, <r,zt>, Z^T zt (K of them), Z^T r (K), <b',b'>
constexpr int kNsSlots = 3 + 2 * kNsMaxK;

struct NullSpace {
    int k = 0;
    bool constant = false;          // Z = 1/sqrt(n): not stored
    double check_tol = 0.0;
    int64_t ld = 0;                 // column stride of Z: n rounded up to an even count (every column 16-byte aligned)
    double *Z = nullptr;            // device, k columns in the HANDLE's numbering (null when constant)
    std::vector<double> Z_host;     // the orthonormal basis, column-major n x k in the CALLER's numbering (empty when constant)
    double *bp = nullptr;           // b' = P b in the handle's numbering
    double *part = nullptr;         // kNsSlots x kMaxGrid
};

namespace {

// out = in - Z (Z^T in) from the partials k_proj_col_dots left (out may be in)
template <int K, bool CONST>
__global__ __launch_bounds__(kBlock) void k_ns_project(int64_t n, const double *in, double *out, const double *__restrict__ Z, int64_t ld,
                                                       double zc, const double *__restrict__ part, int G) {
    __shared__ double sh[4 * K];
    double c[K];
    reduce_slots<K>(part, kProjSlotCols, G, c, sh);
    if (CONST) c[0] = zc * c[0];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double vi = in[i];
#pragma unroll
        for (int j = 0; j < K; ++j) vi = vi - (CONST ? zc : Z[(int64_t)j * ld + i]) * c[j];
        out[i] = vi;
    }
}

// ---- the check of A Z = 0 (setup): workgroup maxima, the host takes the maximum of those -------------------------------------
__device__ __forceinline__ double block_max(double v, double *sh) {      // sh: kBlock doubles; valid in thread 0
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    return sh[0];
}
// out[b] = max over the workgroup's rows of sum_k |a_ik|  (||A||_inf = the maximum over b)
__global__ __launch_bounds__(kBlock) void k_ns_row_abs_max(int64_t n, const int32_t *__restrict__ rp, const double *__restrict__ val,
                                                           double *__restrict__ out) {
    __shared__ double sh[kBlock];
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double s = 0.0;
        for (int k = rp[i]; k < rp[i + 1]; ++k) s += fabs(val[k]);
        m = fmax(m, s);
    }
    m = block_max(m, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}
// out[b] = max |v_i| over the workgroup's rows; a NaN in v comes out as +inf (fmax would drop it)
__global__ __launch_bounds__(kBlock) void k_ns_abs_max(int64_t n, const double *__restrict__ v, double *__restrict__ out) {
    __shared__ double sh[kBlock];
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double a = fabs(v[i]);
        m = (a == a) ? fmax(m, a) : __builtin_huge_val();
    }
    m = block_max(m, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}
__global__ __launch_bounds__(kBlock) void k_ns_fill(int64_t n, double value, double *__restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) v[i] = value;
}

// one basis per shape of Z: the constant column (shape 0), or 1 .. 4 stored ones
struct NullFamily {
    template <class F>
    static void with_shape(int shape, F &&f) {
        if (shape == 0) f(NullBasis<1, true>{});
        else if (shape == 1) f(NullBasis<1, false>{});
        else if (shape == 2) f(NullBasis<2, false>{});
        else if (shape == 3) f(NullBasis<3, false>{});
        else f(NullBasis<4, false>{});
    }
};

inline double z_const(const dpcg_system *h) { return 1.0 / std::sqrt((double)h->A.n); }

ProjectedBasis basis_of(const dpcg_system *h) {
    const NullSpace *ns = h->ns;
    return {ns->constant ? 0 : ns->k, ns->Z, ns->Z, ns->ld, z_const(h), ns->part};
}

// v <- v - Z (Z^T v), or out = in - Z (Z^T in)
void launch_project(const dpcg_system *h, const double *in, double *out, hipStream_t s) {
    const ProjectedBasis pb = basis_of(h);
    const int G = h->vec_grid;
    launch_projected_col_dots<NullFamily>(h, pb, in, pb.k2_cols, s);
    NullFamily::with_shape(pb.shape, [&](auto basis) {
        hipLaunchKernelGGL((k_ns_project<decltype(basis)::K, decltype(basis)::kConst>), dim3(G), dim3(kBlock), 0, s, h->A.n, in, out, pb.k3_cols,
                           pb.ld, pb.zc, pb.part, G);
    });
}

void release(NullSpace *ns) {
    if (!ns) return;
    dev_free(ns->Z);
    dev_free(ns->bp);
    dev_free(ns->part);
    delete ns;
}

// max_i |(A z_j)_i| <= tol ||A||_inf ||z_j||_inf for every column (p, q of the handle are the scratch)
int check_columns(dpcg_system *h, const NullSpace *ns, const std::vector<double> &col_inf, hipStream_t s) {
    const int64_t n = h->A.n;
    const int G = h->vec_grid;
    DPCG_TRY(ensure_work(h, 0, false, false));
    std::vector<double> host((size_t)2 * kMaxGrid, 0.0);
    hipLaunchKernelGGL(k_ns_row_abs_max, dim3(G), dim3(kBlock), 0, s, n, h->A.rowptr, h->A.val, ns->part);
    DPCG_CHECK_LAUNCH();
    DPCG_HIP(hipMemcpyAsync(host.data(), ns->part, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    double norm_a = 0.0;
    for (int i = 0; i < G; ++i) norm_a = std::max(norm_a, host[(size_t)i]);
    for (int j = 0; j < ns->k; ++j) {
        const double *zj = ns->constant ? h->p : ns->Z + (int64_t)j * ns->ld;
        if (ns->constant) hipLaunchKernelGGL(k_ns_fill, dim3(G), dim3(kBlock), 0, s, n, z_const(h), h->p);
        launch_spmv(h->A, h->planA, zj, h->q, nullptr, nullptr, s);
        hipLaunchKernelGGL(k_ns_abs_max, dim3(G), dim3(kBlock), 0, s, n, h->q, ns->part);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipMemcpyAsync(host.data(), ns->part, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        double az = 0.0;
        for (int i = 0; i < G; ++i) az = std::max(az, host[(size_t)i]);
        const double bound = ns->check_tol * norm_a * col_inf[(size_t)j];
        if (!(az <= bound)) {
            char buf[320];
            snprintf(buf, sizeof(buf), "dpcg_set_nullspace: column %d is not in the null space of A: max |A z| = %.3e exceeds check_tol * ||A||_inf * "
                     "||z||_inf = %.3e (check_tol = %.1e)", j, az, bound, ns->check_tol);
            set_error(buf);
            return DPCG_ERR_INVALID;
        }
    }
    return DPCG_OK;
}

std::vector<double> column_inf_norms(const dpcg_system *h, const NullSpace *ns) {
    std::vector<double> out((size_t)ns->k, 0.0);
    const int64_t n = h->A.n;
    if (ns->constant) {
        out[0] = z_const(h);
        return out;
    }
    for (int j = 0; j < ns->k; ++j)
        for (int64_t i = 0; i < n; ++i) out[(size_t)j] = std::max(out[(size_t)j], std::fabs(ns->Z_host[(size_t)j * n + i]));
    return out;
}

}  // namespace
}  // namespace dpcg

void free_nullspace(dpcg_system *h) {
    release(h->ns);
    h->ns = nullptr;
}

const char *nullspace_refusal(const dpcg_system *h, int flags, const double *x_true) {
    if (!h->ns) return nullptr;
    if (flags & DPCG_SINGLE_REDUCTION) return "dpcg_solve: DPCG_SINGLE_REDUCTION is not available on a handle with a null space (the projected recurrence is the standard one)";
    if (flags & DPCG_SPMV_F32) return "dpcg_solve: DPCG_SPMV_F32 is not available on a handle with a null space";
    if (flags & DPCG_TEAM) return "dpcg_solve: DPCG_TEAM is not available on a handle with a null space (no one-launch form projects)";
    if (x_true) return "dpcg_solve: x_true tracking is not available on a handle with a null space (the solution is determined up to the null space)";
    if (h->precond == DPCG_PRECOND_AMG)
        return "dpcg_solve: the AMG preconditioner cannot serve a handle with a null space: its exact coarse solve inverts a singular matrix";
    if (h->precond == DPCG_PRECOND_CALLBACK)
        return "dpcg_solve: the callback preconditioner is not available on a handle with a null space";
    return nullptr;
}

// dpcg_update_values: the null space stays; a check that was asked for is repeated on the new values
int nullspace_values_changed(dpcg_system *h, hipStream_t s) {
    NullSpace *ns = h->ns;
    if (!ns || !(ns->check_tol > 0.0)) return DPCG_OK;
    const int st = check_columns(h, ns, column_inf_norms(h, ns), s);
    if (st == DPCG_ERR_INVALID) {
        std::string msg = dpcg_last_error();
        const std::string from = "dpcg_set_nullspace";
        if (msg.compare(0, from.size(), from) == 0) msg.replace(0, from.size(), "dpcg_update_values (the null space has been dropped)");
        free_nullspace(h);
        set_error(msg);
    }
    return st;
}

extern "C" int dpcg_set_nullspace(dpcg_handle_t h, int k, const double *Z, int memspace, double check_tol, dpcg_stream_t stream) {
    if (!h) return invalid("dpcg_set_nullspace: NULL handle");
    if (k < 0 || k > kNsMaxK) return invalid("dpcg_set_nullspace: k must lie in 0 .. 4 (0 clears)");
    if (k > 0 && h->df) return invalid("dpcg_set_nullspace: the handle has a deflation attached (dpcg_set_deflation): one or the other");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);            // (the old basis may be in use on another stream)
    if (k == 0) {
        free_nullspace(h);
        return DPCG_OK;
    }
    if (!Z && k != 1) return invalid("dpcg_set_nullspace: Z == NULL means the constant vector and needs k == 1");
    if (memspace != DPCG_HOST && memspace != DPCG_DEVICE) return invalid("dpcg_set_nullspace: bad memspace");
    if (!(check_tol == check_tol)) return invalid("dpcg_set_nullspace: check_tol is NaN");
    const int64_t n = h->A.n;
    NullSpace *ns = new NullSpace();
    ns->k = k;
    ns->constant = Z == nullptr;
    ns->check_tol = check_tol;
    ns->ld = (n + 1) & ~(int64_t)1;
    auto fail = [&](int st) {
        release(ns);
        return st;
    };
    int st = DPCG_OK;
    if (!ns->constant) {
        std::vector<double> &Q = ns->Z_host;
        Q.resize((size_t)n * k);
        if (memspace == DPCG_HOST) {
            memcpy(Q.data(), Z, Q.size() * sizeof(double));
        } else {
            hipError_t e = hipMemcpyAsync(Q.data(), Z, Q.size() * sizeof(double), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_nullspace: reading Z", __FILE__, __LINE__));
        }
        for (size_t i = 0; i < Q.size(); ++i)
            if (!std::isfinite(Q[i])) return fail(invalid("dpcg_set_nullspace: Z holds a non-finite entry"));
        // modified Gram-Schmidt in fp64, every column orthogonalised twice against the ones before it
        auto dot = [&](const double *a, const double *b) {
            double acc = 0.0;
            for (int64_t i = 0; i < n; ++i) acc += a[i] * b[i];
            return acc;
        };
        for (int j = 0; j < k; ++j) {
            double *cj = Q.data() + (size_t)j * n;
            const double before = std::sqrt(dot(cj, cj));
            for (int pass = 0; pass < 2; ++pass)
                for (int i = 0; i < j; ++i) {
                    const double *ci = Q.data() + (size_t)i * n;
                    const double c = dot(ci, cj);
                    for (int64_t r = 0; r < n; ++r) cj[r] -= c * ci[r];
                }
            const double after = std::sqrt(dot(cj, cj));
            if (!std::isfinite(after) || !(after > 1e-12 * before)) {
                char buf[200];
                snprintf(buf, sizeof(buf), "dpcg_set_nullspace: Z is rank deficient: column %d has norm %.3e after orthogonalisation, %.3e before", j,
                         after, before);
                set_error(buf);
                return fail(DPCG_ERR_INVALID);
            }
            for (int64_t r = 0; r < n; ++r) cj[r] /= after;
        }
        // to the handle's numbering (row i of the handle = row perm[i] of the caller), columns ld apart, the padding row zero
        std::vector<double> Zp((size_t)ns->ld * k, 0.0);
        std::vector<int32_t> perm;
        if ((st = read_perm(h, perm, s)) < 0) return fail(st);
        for (int j = 0; j < k; ++j)
            for (int64_t i = 0; i < n; ++i) Zp[(size_t)j * ns->ld + i] = Q[(size_t)j * n + (perm.empty() ? i : perm[(size_t)i])];
        if ((st = dev_alloc(&ns->Z, ns->ld * k)) < 0) return fail(st);
        hipError_t e = hipMemcpyAsync(ns->Z, Zp.data(), Zp.size() * sizeof(double), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);       // (Zp goes out of scope)
        if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_nullspace: uploading Z", __FILE__, __LINE__));
    }
    if ((st = dev_alloc(&ns->bp, n)) < 0) return fail(st);
    if ((st = dev_alloc(&ns->part, (int64_t)kNsSlots * kMaxGrid)) < 0) return fail(st);
    if (check_tol > 0.0 && (st = check_columns(h, ns, column_inf_norms(h, ns), s)) < 0) return fail(st);
    free_nullspace(h);
    h->ns = ns;
    return DPCG_OK;
}

extern "C" int dpcg_get_nullspace(dpcg_handle_t h, int *k, double *Z_host) {
    if (!h || !k) return invalid("dpcg_get_nullspace: NULL argument");
    const NullSpace *ns = h->ns;
    *k = ns ? ns->k : 0;
    if (!ns || !Z_host) return DPCG_OK;
    const int64_t n = h->A.n;
    if (ns->constant) {
        const double zc = z_const(h);
        for (int64_t i = 0; i < n; ++i) Z_host[i] = zc;
    } else {
        memcpy(Z_host, ns->Z_host.data(), ns->Z_host.size() * sizeof(double));
    }
    return DPCG_OK;
}

// The solve of a handle with a null space, whatever its size: plain launches enqueued ahead of the progress word that K3 posts
// (the kernels of an update enqueued beyond the stop return at once, as in the definite driver).
int solve_nullspace_one(dpcg_system *h, SolveCall c) {
    NullSpace *ns = h->ns;
    hipStream_t s = c.s;
    const ProjectedBasis pb = basis_of(h);
    const double *bp = nullptr;
    DPCG_TRY(stage_call(h, c.b, c.x0, c.max_iter, false, false, s, &bp, [&](const double *b) {
        launch_project(h, b, ns->bp, s);                                               // b' = P b;  r = b' - A x0
        return (const double *)ns->bp;
    }));
    if (c.x0) launch_project(h, h->r, h->r, s);                                        // r = P r, once
    std::chrono::steady_clock::time_point t0;
    DPCG_TRY(start_projected<NullFamily>(h, pb, bp, c, &t0));
    DPCG_TRY(run_launch_ahead(h, c.max_iter, s, t0, " (null space)", [&] { return enqueue_projected_update<NullFamily>(h, pb, s); }));
    launch_project(h, h->x, h->x, s);                                                  // the minimum-norm solution
    launch_final_check(h->scal, s);
    return deliver_solve(h, c, t0);
}
