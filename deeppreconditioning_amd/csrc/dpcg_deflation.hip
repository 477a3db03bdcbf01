// Deflated PCG (dpcg_set_deflation / dpcg_get_deflation, include/dpcg.h): Saad, Yeung, Erhel, Guyomarc'h, "A deflated version of the
// conjugate gradient algorithm", SISC 21 (2000); with piecewise-constant vectors it is Nicolaides' subdomain deflation.  Not in the
// reference.  Compiled with -ffp-contract=off like dpcg_pcg.hip and dpcg_nullspace.hip.
//
// W is n x k (1 <= k <= 8) with W^T A W = I, AW = A W stored beside it.  The solve (the contract is in include/dpcg.h):
//     start:   r = b - A x0 (x0 NULL: r = b);  c = W^T r;  x = x0 + W c;  r = r - AW c;  z = M r;  mu = AW^T z;  p = z - W mu;  rho = <r,z>
//     update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  z = M r;  mu = AW^T z;  rho' = <r,z>;
//              p = (z - W mu) + (rho'/rho) p
// The recurrence's kernels and the launch of an update are dpcg_projected.h's, over DeflationBasis (U = A W, V = W; rho = <r,z>).
// K2 reads AW and K3 reads W: 8 k bytes per row each on top of the 40 a Jacobi update moves per pass.  The kernels exist for
// 1, 2, 4 and 8 columns; W and AW are stored with that many, the extra columns zero (mu_j = 0 exactly, z - 0 * 0 = z exactly).
// Columns are ld rows apart, ld = n rounded up to a multiple of 1024 (the layout dpcg_guess.hip's CholQR2 kernels run on, which the
// attach shares), the padding rows zero.  Here: the start correction, the A-orthonormalisation, the attach and the solve.
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dpcg_device.h"
#include "dpcg_host.h"
#include "dpcg_projected.h"

namespace dpcg {

constexpr int kDfMaxK = 8;
constexpr int64_t kDfSpan = 1024;             // ld is a multiple of it (dpcg_guess.hip's kernels take whole workgroups of 512 rows)
constexpr double kDfTolDep = 1e-7;            // a column is dependent when its pivot is <= kDfTolDep^2 G_jj (the guess's default)
// partial slots (dpcg_projected.h): <r,r>, <r,z>, AW^T z or W^T r (K of them), <b,b>
constexpr int kDfSlots = 3 + kDfMaxK;
constexpr int kDfCoefGram = 0, kDfCoefRinv = kDfMaxK * kDfMaxK, kDfCoefCount = 2 * kDfMaxK * kDfMaxK;

struct Deflation {
    int k = 0;                      // columns attached
    int kp = 0;                     // columns stored: 1, 2, 4 or 8
    int64_t ld = 0;
    double *W = nullptr;            // device, kp columns in the HANDLE's numbering, W^T A W = I
    double *AW = nullptr;           // A W, the same layout
    double *part = nullptr;         // kDfSlots x kMaxGrid
    double *gs_part = nullptr;      // CholQR2: k x ld / 128 wave partials
    double *coef = nullptr;         // CholQR2: the Gram matrix and R^-1
};

namespace {

// The start correction: after k_proj_col_dots has left the partials of c = W^T r, x += W c and r -= AW c, the columns in ascending order
template <int K>
__global__ __launch_bounds__(kBlock) void k_df_correct(int64_t n, double *__restrict__ x, double *__restrict__ r,
                                                       const double *__restrict__ W, const double *__restrict__ AW, int64_t ld,
                                                       const double *__restrict__ part, int G) {
    __shared__ double sh[4 * K];
    double c[K];
    reduce_slots<K>(part, kProjSlotCols, G, c, sh);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double xi = x[i], ri = r[i];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            xi = xi + W[(int64_t)j * ld + i] * c[j];
            ri = ri - AW[(int64_t)j * ld + i] * c[j];
        }
        x[i] = xi;
        r[i] = ri;
    }
}

// one basis per stored width (the shape)
struct DeflationFamily {
    template <class F>
    static void with_shape(int shape, F &&f) {
        if (shape == 1) f(DeflationBasis<1>{});
        else if (shape == 2) f(DeflationBasis<2>{});
        else if (shape == 4) f(DeflationBasis<4>{});
        else f(DeflationBasis<8>{});
    }
};

ProjectedBasis basis_of(const dpcg_system *h) {
    const Deflation *df = h->df;
    return {df->kp, df->AW, df->W, df->ld, 0.0, df->part};
}

void release(Deflation *df) {
    if (!df) return;
    dev_free(df->W);
    dev_free(df->AW);
    dev_free(df->part);
    dev_free(df->gs_part);
    dev_free(df->coef);
    delete df;
}

// AW = A W by k calls of the handle's SpMV, then CholQR2 in the A inner product, as dpcg_guess.hip does after new values (its device
// pieces): twice G = W^T AW on the device, G = R^T R on the host, W <- W R^-1 and AW <- AW R^-1 in place.  A dependent column -- a
// pivot <= kDfTolDep^2 G_jj -- is refused (`who` names the caller in the text), not dropped.
int a_orthonormalise(dpcg_system *h, Deflation *df, const char *who, hipStream_t s) {
    const int k = df->k;
    DPCG_TRY(ensure_work(h, 0, false, false));
    for (int j = 0; j < k; ++j) launch_spmv(h->A, h->planA, df->W + (int64_t)j * df->ld, df->AW + (int64_t)j * df->ld, nullptr, nullptr, s);
    DPCG_CHECK_LAUNCH();
    std::vector<double> G((size_t)k * k), T;
    for (int round = 0; round < 2; ++round) {
        // column j of the Gram matrix: G[i][j] = <w_i, AW_j>, kept at G[j * k + i]
        for (int j = 0; j < k; ++j)
            gs_gram_column(df->ld, k, df->W, df->AW + (int64_t)j * df->ld, df->gs_part, df->coef + kDfCoefGram + j * k, s);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipMemcpyAsync(G.data(), df->coef + kDfCoefGram, (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        const int keep = gs_cholesky_rinv(G, k, kDfTolDep * kDfTolDep, T);
        if (keep < k) {
            char buf[320];
            snprintf(buf, sizeof(buf), "%s: column %d of W depends on the columns before it in the A inner product (or is zero, or A is not "
                     "positive definite on it): its pivot is <= tol^2 G_jj = %.3e (tol = %.1e)", who, keep,
                     kDfTolDep * kDfTolDep * G[(size_t)keep * k + keep], kDfTolDep);
            set_error(buf);
            return DPCG_ERR_INVALID;
        }
        DPCG_HIP(hipMemcpyAsync(df->coef + kDfCoefRinv, T.data(), (size_t)k * k * sizeof(double), hipMemcpyHostToDevice, s));
        gs_rmul_pair(df->ld, k, df->W, df->AW, df->coef + kDfCoefRinv, s);
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipStreamSynchronize(s));      // (T is overwritten by the next round)
    }
    return DPCG_OK;
}

}  // namespace
}  // namespace dpcg

void free_deflation(dpcg_system *h) {
    release(h->df);
    h->df = nullptr;
}

const char *deflation_refusal(const dpcg_system *h, int flags, const double *x_true) {
    if (!h->df) return nullptr;
    if (flags & DPCG_SINGLE_REDUCTION) return "dpcg_solve: DPCG_SINGLE_REDUCTION is not available on a handle with a deflation (the deflated recurrence is the standard one)";
    if (flags & DPCG_SPMV_F32) return "dpcg_solve: DPCG_SPMV_F32 is not available on a handle with a deflation";
    if (flags & DPCG_TEAM) return "dpcg_solve: DPCG_TEAM is not available on a handle with a deflation (no one-launch form deflates)";
    if (x_true) return "dpcg_solve: x_true tracking is not available on a handle with a deflation";
    if (h->precond == DPCG_PRECOND_CALLBACK)
        return "dpcg_solve: the callback preconditioner is not available on a handle with a deflation (updates are enqueued ahead of the test)";
    if (h->ns) return "dpcg_solve: the handle has both a null space and a deflation";
    return nullptr;
}

// dpcg_update_values: the span stays; A W and the A-orthonormalisation are redone for the new values
int deflation_values_changed(dpcg_system *h, hipStream_t s) {
    if (!h->df) return DPCG_OK;
    const int st = a_orthonormalise(h, h->df, "dpcg_update_values (the deflation has been dropped)", s);
    if (st < 0) free_deflation(h);
    return st;
}

extern "C" int dpcg_set_deflation(dpcg_handle_t h, int k, const double *W, int memspace, dpcg_stream_t stream) {
    if (!h) return invalid("dpcg_set_deflation: NULL handle");
    if (k < 0 || k > kDfMaxK) return invalid("dpcg_set_deflation: k must lie in 0 .. 8 (0 clears)");
    hipStream_t s = (hipStream_t)stream;
    SetupScope scope(s, true);            // (the old vectors may be in use on another stream)
    if (k == 0) {
        free_deflation(h);
        return DPCG_OK;
    }
    if (!W) return invalid("dpcg_set_deflation: W is NULL");
    if (memspace != DPCG_HOST && memspace != DPCG_DEVICE) return invalid("dpcg_set_deflation: bad memspace");
    if (h->ns) return invalid("dpcg_set_deflation: the handle has a null space attached (dpcg_set_nullspace): one or the other");
    const int64_t n = h->A.n;
    if (k > n) return invalid("dpcg_set_deflation: more columns than rows");
    Deflation *df = new Deflation();
    df->k = k;
    df->kp = k <= 2 ? k : (k <= 4 ? 4 : 8);
    df->ld = (n + kDfSpan - 1) / kDfSpan * kDfSpan;
    auto fail = [&](int st) {
        release(df);
        return st;
    };
    std::vector<double> Q((size_t)n * k);
    if (memspace == DPCG_HOST) {
        memcpy(Q.data(), W, Q.size() * sizeof(double));
    } else {
        hipError_t e = hipMemcpyAsync(Q.data(), W, Q.size() * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_deflation: reading W", __FILE__, __LINE__));
    }
    for (size_t i = 0; i < Q.size(); ++i)
        if (!std::isfinite(Q[i])) return fail(invalid("dpcg_set_deflation: W holds a non-finite entry"));
    // to the handle's numbering (row i of the handle = row perm[i] of the caller), columns ld apart, the padding rows and columns zero
    int st = DPCG_OK;
    std::vector<int32_t> perm;
    if ((st = read_perm(h, perm, s)) < 0) return fail(st);
    std::vector<double> Wp((size_t)df->ld * df->kp, 0.0);
    for (int j = 0; j < k; ++j)
        for (int64_t i = 0; i < n; ++i) Wp[(size_t)j * df->ld + i] = Q[(size_t)j * n + (perm.empty() ? i : perm[(size_t)i])];
    const int64_t total = df->ld * df->kp;
    if ((st = dev_alloc(&df->W, total)) < 0 || (st = dev_alloc(&df->AW, total)) < 0) return fail(st);
    if ((st = dev_alloc(&df->part, (int64_t)kDfSlots * kMaxGrid)) < 0) return fail(st);
    if ((st = dev_alloc(&df->gs_part, (int64_t)k * (df->ld / 128))) < 0) return fail(st);
    if ((st = dev_alloc(&df->coef, kDfCoefCount)) < 0) return fail(st);
    hipError_t e = hipMemcpyAsync(df->W, Wp.data(), Wp.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(df->AW, 0, (size_t)total * sizeof(double), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);       // (Wp goes out of scope)
    if (e != hipSuccess) return fail(hip_fail(e, "dpcg_set_deflation: uploading W", __FILE__, __LINE__));
    if ((st = a_orthonormalise(h, df, "dpcg_set_deflation", s)) < 0) return fail(st);
    free_deflation(h);
    h->df = df;
    return DPCG_OK;
}

extern "C" int dpcg_get_deflation(dpcg_handle_t h, int *k, double *W_host, double *AW_host) {
    if (!h || !k) return invalid("dpcg_get_deflation: NULL argument");
    const Deflation *df = h->df;
    *k = df ? df->k : 0;
    if (!df || (!W_host && !AW_host)) return DPCG_OK;
    DPCG_HIP(device_wide_wait());                         // (no stream argument: whatever stream the attach ran on)
    const int64_t n = h->A.n;
    std::vector<int32_t> perm;
    DPCG_TRY(read_perm(h, perm, nullptr));
    std::vector<double> tmp((size_t)n * df->k);
    const size_t width = (size_t)n * sizeof(double), pitch = (size_t)df->ld * sizeof(double);
    for (int which = 0; which < 2; ++which) {
        double *out = which == 0 ? W_host : AW_host;
        if (!out) continue;
        DPCG_HIP(hipMemcpy2D(tmp.data(), width, which == 0 ? df->W : df->AW, pitch, width, (size_t)df->k, hipMemcpyDeviceToHost));
        for (int j = 0; j < df->k; ++j)
            for (int64_t i = 0; i < n; ++i) out[(size_t)j * n + (perm.empty() ? i : perm[(size_t)i])] = tmp[(size_t)j * n + i];
    }
    return DPCG_OK;
}

// The solve of a handle with a deflation, whatever its size: plain launches enqueued ahead of the progress word that K3 posts (the
// kernels of an update enqueued beyond the stop return at once, as in the plain driver).
int solve_deflated_one(dpcg_system *h, SolveCall c) {
    hipStream_t s = c.s;
    const int G = h->vec_grid;
    const ProjectedBasis pb = basis_of(h);
    const double *b = nullptr;
    DPCG_TRY(stage_call(h, c.b, c.x0, c.max_iter, false, false, s, &b));
    launch_projected_col_dots<DeflationFamily>(h, pb, h->r, pb.k3_cols, s);             // c = W^T r;  x += W c;  r -= AW c
    DeflationFamily::with_shape(pb.shape, [&](auto basis) {
        hipLaunchKernelGGL((k_df_correct<decltype(basis)::K>), dim3(G), dim3(kBlock), 0, s, h->A.n, h->x, h->r, pb.k3_cols, pb.k2_cols, pb.ld,
                           pb.part, G);
    });
    std::chrono::steady_clock::time_point t0;
    DPCG_TRY(start_projected<DeflationFamily>(h, pb, b, c, &t0));
    DPCG_TRY(run_launch_ahead(h, c.max_iter, s, t0, " (deflation)", [&] { return enqueue_projected_update<DeflationFamily>(h, pb, s); }));
    launch_final_check(h->scal, s);
    return deliver_solve(h, c, t0);
}
