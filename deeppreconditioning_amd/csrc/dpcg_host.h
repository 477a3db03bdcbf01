// Host-side internals shared by dpcg_api.hip, dpcg_precond.hip, dpcg_solve.hip and dpcg_solve_chip.hip (not part of the ABI).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dpcg_internal.h"
#include "dpcg_prims.h"

using namespace dpcg;

#define DPCG_TRY(expr)               \
    do {                             \
        int _st = (expr);            \
        if (_st < 0) return _st;     \
    } while (0)

#define DPCG_CHECK_LAUNCH() DPCG_HIP(hipGetLastError())

// sets dpcg_last_error() and returns DPCG_ERR_INVALID
int invalid(const char *msg);

// DPCG_SETUP_TRACE=1: phase times of the setup routines on stderr (development)
struct PhaseTimer {
    bool on;
    hipStream_t s;
    std::chrono::steady_clock::time_point t;
    explicit PhaseTimer(hipStream_t stream) : s(stream) {
        static const bool enabled = [] { const char *e = getenv("DPCG_SETUP_TRACE"); return e && e[0] == '1'; }();
        on = enabled;
        if (on) {
            (void)hipStreamSynchronize(s);
            t = std::chrono::steady_clock::now();
        }
    }
    void mark(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[dpcg setup] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// ---- device memory ---------------------------------------------------------------------------------------
template <typename T>
inline int dev_alloc(T **p, int64_t count) {
    *p = nullptr;
    if (count <= 0) count = 1;
    hipError_t e = cached_alloc((void **)p, (size_t)count * sizeof(T));
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? DPCG_ERR_NOMEM : DPCG_ERR_HIP;
    }
    return DPCG_OK;
}

template <typename T>
inline void dev_free(T *&p) {
    if (p) cached_free(p);
    p = nullptr;
}

// scoped device allocation for the setup routines
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { dev_free(p); }
    int alloc(int64_t count) { dev_free(p); return dev_alloc(&p, count); }
    T *release() { T *q = p; p = nullptr; return q; }
};

// host[0 .. count) = dev[0 .. count), complete on return
template <typename T>
inline int fetch(T *host, const T *dev, int64_t count, hipStream_t s) {
    DPCG_HIP(hipMemcpyAsync(host, dev, (size_t)count * sizeof(T), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

// ---- launch geometry of the setup kernels: workgroups of per_block items that stride over `count` items, at most `cap` of them
inline int grid_blocks(int64_t count, int cap, int per_block = kBlock) {
    const int64_t g = (count + per_block - 1) / per_block;
    return (int)std::min<int64_t>(std::max<int64_t>(g, 1), cap);
}

void free_csr(CsrDev &c);
// dpcg_icholt.hip: ILU++-style thresholded incomplete Cholesky of a symmetric CSR matrix into an owned lower-triangular CSR
// info: {form (1 LDS pipeline, 2 workspace pipeline, 3 one-wave), waves of the pipeline that produced Lf (0: one-wave), the column at
// which a pipeline attempt gave the factorisation to the one-wave kernel (-1: none did), the pool bound} -- dpcg_get_icholt_info
int icholt_factor(const CsrDev &A, int add_fill_in, double threshold, CsrDev &Lf, hipStream_t s, int32_t info[4]);
// dpcg_ilut.hip: Saad's dual-threshold ILUT of a CSR matrix into owned L (unit lower, diagonal last) and U (upper, diagonal first)
int ilut_factor(const CsrDev &A, int add_fill_in, double threshold, CsrDev &Lf, CsrDev &Uf, hipStream_t s);
// dpcg_fsai.hip: the factorised sparse approximate inverse of the handle's matrix (caller's numbering) into an owned lower-triangular
// CSR; level 1 .. 3, or 0 with an explicit lower pattern on the device (taken over).  The handle's FsaiCache serves and is refreshed.
int fsai_factor(dpcg_system *h, int level, int64_t pat_nnz, int32_t *pat_rp, int32_t *pat_ci, CsrDev &Lf, hipStream_t s);
int fsai_upload_pattern(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, int memspace, int32_t **rp_out, int32_t **ci_out,
                        hipStream_t s);
void free_fsai(FsaiCache *&c);
void fsai_detach(FsaiCache *c);                         // the handle's preconditioner is no longer this factor
void fsai_mark_attached(FsaiCache *c);
// dpcg_block_ic.hip: the block-Jacobi incomplete Cholesky -- release; the handle's preconditioner is no longer this factor; the handle has
// been renumbered (the way into its vectors is rebuilt, the factor stays attached); the apply (part_rz: the workgroups leave their
// shares of <r, z>); how many partials an in-loop apply leaves (0: none, more blocks than the partial buffer holds); nnz(L); the getters
void free_block_ic(BlockIc *&c);
void block_ic_detach(BlockIc *c);
int block_ic_renumbered(dpcg_system *h, hipStream_t s);
int block_ic_apply(dpcg_system *h, const double *r, double *z, hipStream_t s, double *part_rz, int *n_part_rz, const int *done = nullptr);
int block_ic_rz_partials(const BlockIc *c);
int64_t block_ic_nnz(const BlockIc *c);
int block_ic_get_factor(const dpcg_system *h, int32_t *rowptr, int32_t *col, double *val);
int block_ic_get_ordering(const dpcg_system *h, int32_t *perm_host);
void free_parked(dpcg_system *h);                       // dpcg_api.hip: the multicolour IC(0) parked by dpcg_update_values
void free_levels(Levels &l);
namespace dpcg { void orphan_guesses(dpcg_system *h); }   // dpcg_guess.hip: the handle is going away
int count_levels_on_demand(dpcg_system *h);   // dpcg_precond.hip
void free_plan(SpmvPlan &plan);
void free_ell(SmallEll &e);
int grid_for(int64_t n);
int upload_csr(CsrDev &out, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, const void *val,
               int val_dtype, int memspace, int copy, hipStream_t s);
// Chooses the SpMV kernel of a matrix (gather / vector / x-tile) and builds the tile plan where it applies.
int make_plan(const CsrDev &A, SpmvPlan &plan, hipStream_t s, bool allow_tile = false);

// ---- handle ----------------------------------------------------------------------------------------------
struct HandleExtras {
    hipStream_t cap_stream = nullptr;
    unsigned long long *prog_host = nullptr;  // pinned + mapped: the solve's progress word
    unsigned long long *prog_dev = nullptr;   // device-side address of the same word
};
// kept outside dpcg_system so the struct in the header stays POD-like; the registry itself is guarded so that
// handles may be created/destroyed from several host threads (one handle is still used by one thread at a time)
struct ExtrasRegistry {
    std::mutex mu;
    std::map<dpcg_system *, HandleExtras> m;
    HandleExtras &operator[](dpcg_system *h) {
        std::lock_guard<std::mutex> lock(mu);
        return m[h];   // std::map nodes are stable: the reference stays valid while the handle lives
    }
    bool take(dpcg_system *h, HandleExtras &out) {
        std::lock_guard<std::mutex> lock(mu);
        auto it = m.find(h);
        if (it == m.end()) return false;
        out = it->second;
        m.erase(it);
        return true;
    }
};
ExtrasRegistry &extras();
void drop_graph(dpcg_system *h);
void free_precond(dpcg_system *h, bool keep_parked = false);   // (by default a parked factor goes too)
// work vectors, partial buffers, history (grown on demand)
int ensure_work(dpcg_system *h, int max_iter, bool need_f32, bool need_err);
// whether a solve with these flags runs two-kernel updates, and the extra operands of its SpMV kernel
bool fuse_eligible(const dpcg_system *h, int flags, const double *x_true);
FuseArgs fuse_args(dpcg_system *h);
// z = M r for the handle's preconditioner (cg.py:61,81); in_loop: kernels return at once when the solve is done
// part_rz / n_part_rz (may be null): where the apply may leave per-workgroup partials of <r,z> (cg.py:82) when its last kernel
// can sum them on the way; *n_part_rz = their count, or 0 when the caller has to launch the dot product itself
// lower_first_done: the first level of the lower solve has been computed already (colour sweeps: it rode on K2)
int apply_precond(dpcg_system *h, const double *r, double *z, hipStream_t s, bool in_loop = false, double *part_rz = nullptr,
                  int *n_part_rz = nullptr, bool lower_first_done = false);
// number of <r,z> partials an in-loop apply of the handle's preconditioner leaves (vec_grid when it leaves none)
int rz_partial_count(const dpcg_system *h);
int check_spin_errors(dpcg_system *h, hipStream_t s);

// ---- the one-launch forms (dpcg_solve.hip: one workgroup, one team; dpcg_solve_chip.hip: the whole chip) --------------------------------
bool device_has_cus(int cus);
std::mutex &team_launch_mutex();          // one team / whole-chip launch at a time per process
// Back-off of the one-launch forms (one workgroup team / whole chip): they assume that all of their workgroups become co-resident, and
// a launch that cannot (RCCL kernels or another process holding CUs, a long kernel on another stream) spins for the full 20 ms bound
// before the call goes on through the launches.  Three such timeouts in a row and the one-launch forms are skipped for a cool-down
// (2 s, doubling up to 32 s while the re-probes keep failing); a launch that completes clears it.  One warning per process.
struct CoResidency {
    std::atomic<int> misses{0};
    std::atomic<long long> closed_until_ns{0};
    std::atomic<int> cooldown_s{2};
    std::atomic<bool> warned{false};
    static long long now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    bool open() const { return now_ns() >= closed_until_ns.load(std::memory_order_relaxed); }
    void launched_fine() {
        misses.store(0, std::memory_order_relaxed);
        cooldown_s.store(2, std::memory_order_relaxed);
    }
    void timed_out() {
        if (misses.fetch_add(1, std::memory_order_relaxed) + 1 < 3) return;
        const int cd = cooldown_s.load(std::memory_order_relaxed);
        closed_until_ns.store(now_ns() + (long long)cd * 1000000000ll, std::memory_order_relaxed);
        cooldown_s.store(std::min(2 * cd, 32), std::memory_order_relaxed);
        misses.store(2, std::memory_order_relaxed);            // (the re-probe after the cool-down closes it again at its first timeout)
        if (!warned.exchange(true))
            fprintf(stderr, "[dpcg] the one-launch solve kernels could not become co-resident three times in a row (somebody else holds CUs): "
                            "solving through the multi-launch path, re-probing every %d s and up\n", cd);
    }
};
CoResidency &co_residency();
// which systems take a whole-chip form, whether a plain call does, and why DPCG_SINGLE_REDUCTION cannot be honoured (nullptr: it can)
bool chip_eligible(const dpcg_system *h, int flags, const double *x_true);
bool chip_llt_eligible(const dpcg_system *h, int flags, const double *x_true);
bool chip_trsv_shape(const dpcg_system *h, int flags, const double *x_true);
bool chip_default(const dpcg_system *h, int flags);
const char *chip_sr_refusal(const dpcg_system *h, int flags, const double *x_true);
void free_chip_trsv(dpcg_system *h);               // the plan of the triangular-solve form (goes with the preconditioner)
// one solve as dpcg_solve takes it (b, x0 and x in the caller's numbering; everything from iters on may be null): the record every form,
// its descriptor and its tail take
struct SolveCall {
    const double *b, *x0;
    double *x;
    double rtol_sq, atol_sq;
    int max_iter, flags;
    hipStream_t s;
    int *iters;
    double *final_res, *seconds, *res_history;
    const double *x_true = nullptr;       // (the launch path only: every other form refuses a call that tracks the error)
    double *err_history = nullptr;
};
// ... by a whole-chip form; DPCG_ERR_STATE: not taken (refused up front, or never co-resident), the caller goes on with the launches
int solve_chip_one(dpcg_system *h, SolveCall c);          // M = I / Jacobi
int solve_chip_sr_one(dpcg_system *h, SolveCall c);       // ... with the single-reduction recurrence
int solve_chip_llt_one(dpcg_system *h, SolveCall c);      // M = L L^T multiplied
int solve_chip_trsv_one(dpcg_system *h, SolveCall c);     // M = (L L^T)^-1 by two triangular solves
// The end of a one-launch solve (one workgroup, one team, the whole chip) whose kernel was enqueued at t0: the scalars, ONE synchronise,
// the timer, the launch check; never_resident (null: the one-workgroup form, no co-residency to account for): the error of a launch whose
// workgroups waited in vain, co_residency() is told either way; ran(sc), if any, after a launch that ran; then deliver_results with x in
// place.  Returns the solve's status.
int finish_one_launch(dpcg_system *h, const SolveCall &c, std::chrono::steady_clock::time_point t0, const char *never_resident,
                      const std::function<int(const Scalars &)> &ran = nullptr);
// ---- the pieces of a launch-path solve (dpcg_solve.hip), shared by the plain driver, the two projected ones and dpcg_solve_refined; the
// ---- last three of them (deliver_results, hand_over_x, gather_rhs) by the one-launch forms too ----------------------------------------
// how the vector kernels see M: 0 = I, 1 = Jacobi (z = dinv r on the fly), 2 = anything else (an apply between K2 and K3)
inline int precond_class(const dpcg_system *h) { return h->precond == DPCG_PRECOND_NONE ? 0 : (h->precond == DPCG_PRECOND_JACOBI ? 1 : 2); }
// the handle's permutation on the host (empty: the handle is not reordered)
int read_perm(const dpcg_system *h, std::vector<int32_t> &perm, hipStream_t s);
// Staging of a call, in two parts.  stage_vectors: the work vectors, the progress word zeroed, b gathered into the handle's numbering
// (*b_used), x = x0 or 0 -- all dpcg_solve_refined takes, it forms its own residual.  stage_residual: r = b - A x or r = b.
// stage_call: both; rhs (may be empty) is called with the gathered b in between and returns the right-hand side to use in its place
// (*b_used: that one).
int stage_vectors(dpcg_system *h, const double *b, const double *x0, int max_iter, bool need_f32, bool need_err, hipStream_t s,
                  const double **b_used);
int stage_residual(dpcg_system *h, const double *b, bool have_x0, hipStream_t s);
int stage_call(dpcg_system *h, const double *b, const double *x0, int max_iter, bool need_f32, bool need_err, hipStream_t s,
               const double **b_used, const std::function<const double *(const double *)> &rhs = nullptr);
// Waits until the progress word leaves v -- a bounded spin, then a look at the stream so that a fault cannot hang the host.  Returns
// DPCG_OK (moved, or still running: the caller looks again) or the error; behind: updates are enqueued beyond the one v reports, so a
// drained stream must have moved the word.  tag: "", " (null space)", " (deflation)".
int wait_progress(volatile unsigned long long *prog, unsigned long long v, hipStream_t s, bool behind, const char *tag);
// Plain launches kept enqueued ahead of the progress word until the solve reports its end or max_iter: 16 updates before the time
// per update is known (from the fourth on), then enough to cover ~150 us of host latency, 3 .. 32.
int run_launch_ahead(dpcg_system *h, int max_iter, hipStream_t s, std::chrono::steady_clock::time_point t0, const char *tag,
                     const std::function<int()> &enqueue_update);
// The delivery tail, after the finaliser has been enqueued: the scalars, the end of the timer (c.seconds counts from t0), errors of the
// sync-free triangular solves (which only this path can meet), then deliver_results.  Returns the solve's status.
int deliver_solve(dpcg_system *h, const SolveCall &c, std::chrono::steady_clock::time_point t0);
// What every tail ends in: iters / final_res / seconds, res_history (a second synchronise only when it was asked for), x handed over in
// stream order (hand_over_x: h->x to the caller's x and numbering) unless the kernel wrote it in place and the handle is not reordered.
int deliver_results(dpcg_system *h, const SolveCall &c, const Scalars &sc, double seconds, bool x_in_place);
int hand_over_x(dpcg_system *h, double *x, hipStream_t s);
// b into the handle's numbering (h->pb) where the handle is reordered
int gather_rhs(dpcg_system *h, const double *&b, hipStream_t s);
// dpcg_nullspace.hip: singular systems with an attached null space (dpcg_set_nullspace).  Why a solve with these arguments is refused
// (nullptr: it is not); the solve itself, whatever the system's size; the check of A Z = 0 again after dpcg_update_values; the release
const char *nullspace_refusal(const dpcg_system *h, int flags, const double *x_true);
int solve_nullspace_one(dpcg_system *h, SolveCall c);
int nullspace_values_changed(dpcg_system *h, hipStream_t s);
void free_nullspace(dpcg_system *h);
// dpcg_deflation.hip: deflated PCG (dpcg_set_deflation), the same four -- after dpcg_update_values A W and the A-orthonormalisation are redone
const char *deflation_refusal(const dpcg_system *h, int flags, const double *x_true);
int solve_deflated_one(dpcg_system *h, SolveCall c);
int deflation_values_changed(dpcg_system *h, hipStream_t s);
void free_deflation(dpcg_system *h);
// dpcg_refine.hip: what dpcg_solve_refined keeps on the handle (fp32 values, fp32 reciprocal diagonal, fp32 work vectors); free_precond
// calls it, so new values, a new preconditioner and a reordering all drop it
void free_refine(dpcg_system *h);
// dpcg_bicgstab.hip: what dpcg_solve_bicgstab keeps on the handle (four work vectors, partial buffers, its scalar record); dpcg_destroy
// calls it
void free_bicgstab(dpcg_system *h);
// dpcg_guess.hip, shared with dpcg_deflation.hip: the device and host pieces of CholQR2 on a tall-skinny pair X, W = A X (column-major, ld a
// multiple of 1024 rows apart, padding rows zero).  gs_gram_column: out[i] = <X[:, i], v>, i < l (part: l x ld / 128 doubles of scratch);
// gs_cholesky_rinv: G = R^T R (G[j * l + i] = G_ij), T = R^-1 of the leading keep x keep block (row-major), keep = the first j whose pivot is
// <= tol2 G_jj (l: none); gs_rmul_pair: X <- X T, W <- W T in place (T on the device).
void gs_gram_column(int64_t ld, int l, const double *X, const double *v, double *part, double *out, hipStream_t s);
int gs_cholesky_rinv(const std::vector<double> &G, int l, double tol2, std::vector<double> &T);
void gs_rmul_pair(int64_t ld, int l, double *X, double *W, const double *rinv, hipStream_t s);
// dpcg_amg.hip: the smoothed-aggregation hierarchy -- free, launches of one V-cycle, sum over levels of nnz(A_l) + 2 nnz(P_l), the apply
// (part_rz: the last kernel leaves the partials of <r, z>), and how many partials an in-loop apply leaves (0: none)
void free_amg(AmgState *&S);
int amg_launches(const AmgState *S);
int64_t amg_nnz(const AmgState *S);
int amg_apply(dpcg_system *h, const double *r, double *z, hipStream_t s, double *part_rz, int *n_part_rz, const int *done = nullptr);
int amg_rz_partials(const AmgState *S);
