// Host side of libdpcg.so, part 3: the PCG driver -- enqueues the iteration kernels (as replayed hipGraph chunks or
// update by update) ahead of a progress word the GPU posts to pinned memory, the whole-solve kernels for small and mid-size
// systems (one workgroup, one team), the dispatch between the forms and the batch entry point.  The whole-chip forms:
// dpcg_solve_chip.hip.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "dpcg_host.h"
#include "dpcg_prims.h"
#include "dpcg_stream_set.h"

// ------------------------------------------------------------------------------------------------
// the solve
// ------------------------------------------------------------------------------------------------
static int default_chunk() {
    const char *e = getenv("DPCG_CHUNK");
    int c = e ? atoi(e) : 8;
    return c < 1 ? 1 : (c > 256 ? 256 : c);
}

// The x update is deferred to every second update (k_update_xp_deferred) in the three-kernel form; x_true tracking
// needs x after every update.
static bool defer_x_eligible(const dpcg_system *h, int flags, const double *x_true) {
    static const bool enabled = [] { const char *e = getenv("DPCG_DEFER_X"); return !(e && e[0] == '0'); }();
    return enabled && !x_true && !fuse_eligible(h, flags, x_true);
}

// The vector kernels of a system whose streams exceed the Infinity Cache (the x-tile SpMV reads them non-temporally: 256^3) store what
// they produce non-temporally too.  DPCG_VEC_NT=0/1: development knob.
static bool vec_nt(const dpcg_system *h) {
    static const int knob = [] { const char *e = getenv("DPCG_VEC_NT"); return e ? atoi(e) : -1; }();
    return knob >= 0 ? knob != 0 : (h->planA.kernel == SPMV_TILE && h->planA.stream_nt);
}

// One PCG update (cg.py:75-86) as kernel launches on `s`; `j` = index of this update within the solve (its parity
// selects the p buffer in the deferred-x form: a replayed graph chunk has an even length and starts at an even j).
static int enqueue_iteration(dpcg_system *h, int flags, const double *x_true, hipStream_t s, int j) {
    const int64_t n = h->A.n;
    const bool f32 = (flags & DPCG_SPMV_F32) != 0;
    // colour sweeps: the first level of the lower solve (rows without dependencies: y = r / d) rides on the kernel that updates r
    const bool ride = h->precond == DPCG_PRECOND_LLT_SOLVE && h->lvlL.sweep && h->lvlL.ride_diag && h->lvlL.n_levels >= 2;
    if (fuse_eligible(h, flags, x_true)) {
        // KA: test of the current iterate, p = z + beta p, deferred x += alpha p, q = A p, partials of <p,q>
        launch_spmv_fused(h->A, h->planA, fuse_args(h), h->q, h->part_pq, h->scal, s);          // cg.py:71,83,79,75
        // KB: alpha; r -= alpha q; (z = M r fused); partials <r,z>, <r,r>; k += 1                cg.py:78,80-82,86
        const int pre = precond_class(h);
        if (ride)
            launch_update_r_ride(n, h->scal, h->part_pq, h->planA.grid, h->q, h->r, h->lvlL.ride_diag, h->lvlL.lm_pos, h->lvlL.lm_out,
                                 h->lvlL.level_ptr[1], h->part_rr, h->vec_grid, s, true);
        else
            launch_update_r_two_kernel(pre, n, h->scal, h->part_pq, h->planA.grid, h->q, h->r, h->dinv, h->z, h->part_rz,
                                       h->part_rr, h->vec_grid, s);
        if (pre == 2) {
            int np = 0;
            DPCG_TRY(apply_precond(h, h->r, h->z, s, true, h->part_rz, &np, ride));              // cg.py:81 (+ cg.py:82 when fused)
            if (np == 0) launch_dot_partials(n, h->scal, h->r, h->z, h->part_rz, h->vec_grid, s);   // cg.py:82
        }
        return DPCG_OK;
    }
    IterCtl ctl{h->scal};
    // K1: (skip when done) Ap = A p + partials of <p,Ap>           cg.py:71,75,78
    const bool v32 = !f32 && (flags & DPCG_VAL32_IF_LOSSLESS) && h->A.val32_lossless == 1;
    const bool defer_x = defer_x_eligible(h, flags, x_true);
    double *p_cur = (defer_x && (j & 1)) ? h->p2 : h->p;               // p_j
    double *p_next = (defer_x && !(j & 1)) ? h->p2 : h->p;             // where p_{j+1} goes (in place without deferral)
    if (f32) launch_spmv_f32in(h->A, h->planA, h->p32, p_cur, h->q, h->part_pq, &ctl, s);
    else if (v32) launch_spmv_val32(h->A, h->planA, p_cur, h->q, h->part_pq, &ctl, s);
    else launch_spmv(h->A, h->planA, p_cur, h->q, h->part_pq, &ctl, s);
    // K2: alpha; r -= alpha Ap; (z = M r fused); partials <r,z>, <r,r>              cg.py:78,80-82,86
    const int pre = precond_class(h);
    // Jacobi: z = dinv .* r is never stored -- K2 only needs it for <r,z>, and K3 recomputes the same product from r and
    // dinv (same rounding, same bits).  That moves 8 B per row from a write in K2 to a read in K3; writes are the dearer
    // direction (measured: 34.9 -> 33.1 us per update at 1M DoF).
    const bool z_on_the_fly = pre == 1;
    const double *z = pre == 2 ? h->z : h->r;
    if (ride)
        launch_update_r_ride(n, h->scal, h->part_pq, h->planA.grid, h->q, h->r, h->lvlL.ride_diag, h->lvlL.lm_pos, h->lvlL.lm_out,
                             h->lvlL.level_ptr[1], h->part_rr, h->vec_grid, s);
    else
        launch_update_r(pre, n, h->scal, h->part_pq, h->planA.grid, h->q, h->r, h->dinv, h->z, h->part_rz, h->part_rr,
                        h->vec_grid, s, z_on_the_fly ? 0 : 1, vec_nt(h));
    const int np_rz = pre == 2 ? rz_partial_count(h) : h->vec_grid;
    if (pre == 2) {
        int np = 0;
        DPCG_TRY(apply_precond(h, h->r, h->z, s, true, h->part_rz, &np, ride));      // cg.py:81 (+ cg.py:82 when fused)
        if (np == 0) launch_dot_partials(n, h->scal, h->r, h->z, h->part_rz, h->vec_grid, s);   // cg.py:82
    }
    // K3: beta; x += alpha p; p = z + beta p; workgroup 0: stopping test of the new iterate   cg.py:79,82-83,86,71
    if (defer_x)
        launch_update_xp_deferred((j & 1) != 0, n, h->scal, h->part_rz, h->part_rr, np_rz, z, p_cur, p_next, h->x,
                                  f32 ? h->p32 : nullptr, h->hist, h->hist_cap, h->vec_grid, s,
                                  z_on_the_fly ? h->dinv : nullptr, h->vec_grid, vec_nt(h));
    else
        launch_update_xp(n, h->scal, h->part_rz, h->part_rr, np_rz, z, h->p, h->x, f32 ? h->p32 : nullptr, h->hist,
                         h->hist_cap, h->vec_grid, s, z_on_the_fly ? h->dinv : nullptr, h->vec_grid);
    if (x_true) {                                                                    // cg.py:43-45
        launch_anorm_err(n, h->scal, h->x, x_true, h->e, h->vec_grid, s);
        launch_spmv(h->A, h->planA, h->e, h->t, h->part_bb, nullptr, s);
        launch_record_err(h->scal, h->part_bb, h->planA.grid, h->err_hist, h->hist_cap, 0, s);
    }
    return DPCG_OK;
}

static int ensure_graph(dpcg_system *h, int flags, int chunk) {
    const int key = (h->precond << 8) | (flags & (DPCG_SPMV_F32 | DPCG_VAL32_IF_LOSSLESS | DPCG_NO_FUSE)) |
                    (h->A.val32_lossless == 1 ? 64 : 0) | (fuse_eligible(h, flags, nullptr) ? 128 : 0) |
                    (defer_x_eligible(h, flags, nullptr) ? 1024 : 0) | (vec_nt(h) ? 2048 : 0);
    if (h->graph_exec && h->graph_key == key && h->graph_chunk == chunk) return DPCG_OK;
    drop_graph(h);
    HandleExtras &ex = extras()[h];
    hipGraph_t graph = nullptr;
    int st = DPCG_OK;
    hipError_t e = hipSuccess;
    {
        CaptureGuard no_device_wide_waits_meanwhile;          // (another host thread's hipFree / hipDeviceSynchronize would void the capture)
        // (relaxed mode: what OTHER host threads call meanwhile -- torch allocating or synchronising -- is their business; the
        // capture stream itself is private to this handle)
        DPCG_HIP(hipStreamBeginCapture(ex.cap_stream, hipStreamCaptureModeRelaxed));
        for (int i = 0; i < chunk && st >= 0; ++i) st = enqueue_iteration(h, flags, nullptr, ex.cap_stream, i);
        e = hipStreamEndCapture(ex.cap_stream, &graph);
    }
    if (e != hipSuccess) {
        // The capture was voided from outside -- HIP refuses a device-wide wait while ANY stream captures, and void-s the capture
        // too: another host thread of the application calling torch.cuda.synchronize() at that moment does it
        // (tools/thread_probe.py).  Not an error of this solve: it runs update by update, the next one captures again.
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        return DPCG_OK;                                  // (h->graph_exec stays null: the caller checks)
    }
    if (st < 0) {
        if (graph) (void)hipGraphDestroy(graph);
        return st;
    }
    e = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    DPCG_HIP(e);
    h->graph_key = key;
    h->graph_chunk = chunk;
    return DPCG_OK;
}

// kernel launches one preconditioner application costs (the SpTRSVs launch once per wide level)
static int precond_launches(const dpcg_system *h) {
    auto trsv = [](const Levels &lv) {
        if (lv.strips.n_strips > 0) return 2;
        int c = 0;
        for (const auto &seg : lv.segments) c += (seg.merged || seg.syncfree) ? 2 : seg.hi - seg.lo;
        return c;
    };
    switch (h->precond) {
        case DPCG_PRECOND_CSR: return 1;
        case DPCG_PRECOND_CALLBACK: return 1;
        case DPCG_PRECOND_LLT_MULTIPLY: case DPCG_PRECOND_LU_MULTIPLY: return 2;
        case DPCG_PRECOND_LLT_SOLVE: case DPCG_PRECOND_LU_SOLVE: return trsv(h->lvlL) + trsv(h->lvlU);
        case DPCG_PRECOND_AMG: return amg_launches(h->amg);
        case DPCG_PRECOND_BLOCK_LLT_SOLVE: return 1;
        default: return 0;
    }
}

// A sync-free triangular solve whose bounded poll ran out (cannot happen with a schedule built by this library) has
// stored NaNs; report it instead of a silent breakdown.
int check_spin_errors(dpcg_system *h, hipStream_t s) {
    if (h->precond != DPCG_PRECOND_LLT_SOLVE && h->precond != DPCG_PRECOND_LU_SOLVE) return DPCG_OK;
    for (Levels *lv : {&h->lvlL, &h->lvlU}) {
        if (!lv->spin_err) continue;
        int e = 0;
        DPCG_HIP(hipMemcpyAsync(&e, lv->spin_err, sizeof(int), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        if (e) {
            (void)hipMemsetAsync(lv->spin_err, 0, sizeof(int), s);
            // the failed solve stored NaNs: put the "all pending between solves" invariant of the lower factor's level-major
            // solution vector back (Levels::lm_out), so that the handle stays usable
            if (single_syncfree_segment(h->lvlL) && h->lvlL.lm_out) launch_fill_pending(h->lvlL.lm_out, h->A.n, s);
            (void)hipStreamSynchronize(s);
            set_error("sync-free triangular solve: a row waited (4 s) for an entry that was never written");
            return DPCG_ERR_STATE;
        }
    }
    return DPCG_OK;
}

int read_perm(const dpcg_system *h, std::vector<int32_t> &perm, hipStream_t s) {
    perm.clear();
    if (!h->perm) return DPCG_OK;
    perm.resize((size_t)h->A.n);
    DPCG_HIP(hipMemcpyAsync(perm.data(), h->perm, perm.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    return DPCG_OK;
}

int gather_rhs(dpcg_system *h, const double *&b, hipStream_t s) {
    if (!h->perm) return DPCG_OK;          // (b arrives in the caller's numbering)
    if (!h->pb) DPCG_TRY(dev_alloc(&h->pb, h->A.n));
    launch_gather_f64(h->A.n, h->perm, b, h->pb, s);
    b = h->pb;
    return DPCG_OK;
}

int stage_vectors(dpcg_system *h, const double *b, const double *x0, int max_iter, bool need_f32, bool need_err, hipStream_t s,
                  const double **b_used) {
    const int64_t n = h->A.n;
    DPCG_TRY(ensure_work(h, max_iter, need_f32, need_err));
    *extras()[h].prog_host = 0;
    DPCG_TRY(gather_rhs(h, b, s));
    if (!x0) DPCG_HIP(hipMemsetAsync(h->x, 0, (size_t)n * sizeof(double), s));       // cg.py:58
    else if (h->perm) launch_gather_f64(n, h->perm, x0, h->x, s);                    // (x0 arrives in the caller's numbering too)
    else DPCG_HIP(hipMemcpyAsync(h->x, x0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    *b_used = b;
    return DPCG_OK;
}

int stage_residual(dpcg_system *h, const double *b, bool have_x0, hipStream_t s) {
    if (have_x0) {
        launch_spmv(h->A, h->planA, h->x, h->q, nullptr, nullptr, s);
        launch_residual(h->A.n, b, h->q, h->r, h->vec_grid, s);                      // cg.py:60
    } else {
        DPCG_HIP(hipMemcpyAsync(h->r, b, (size_t)h->A.n * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    return DPCG_OK;
}

int stage_call(dpcg_system *h, const double *b, const double *x0, int max_iter, bool need_f32, bool need_err, hipStream_t s,
               const double **b_used, const std::function<const double *(const double *)> &rhs) {
    DPCG_TRY(stage_vectors(h, b, x0, max_iter, need_f32, need_err, s, b_used));
    if (rhs) *b_used = rhs(*b_used);
    return stage_residual(h, *b_used, x0 != nullptr, s);
}

int wait_progress(volatile unsigned long long *prog, unsigned long long v, hipStream_t s, bool behind, const char *tag) {
    for (int spin = 0; spin < 4000; ++spin) {
        if (*prog != v) return DPCG_OK;
        __builtin_ia32_pause();
    }
    const hipError_t q = hipStreamQuery(s);
    if (q == hipErrorNotReady) return DPCG_OK;
    DPCG_HIP(q);
    // stream drained: every enqueued update has run, the word is final for them
    if (*prog == v && behind) {
        set_error(std::string("PCG driver") + tag + ": enqueued updates finished without reporting progress");
        return DPCG_ERR_STATE;
    }
    return DPCG_OK;
}

int run_launch_ahead(dpcg_system *h, int max_iter, hipStream_t s, std::chrono::steady_clock::time_point t0, const char *tag,
                     const std::function<int()> &enqueue_update) {
    volatile unsigned long long *prog = extras()[h].prog_host;
    int enq = 0;
    double t_iter = 0.0;
    for (;;) {
        const unsigned long long v = *prog;
        const int k = (int)(v >> 1);
        if ((v & 1ull) || k >= max_iter) return DPCG_OK;
        if (k >= 4) t_iter = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / k;
        // updates kept enqueued beyond the last one reported: enough to cover ~150 us of host latency
        int ahead = 16;
        if (t_iter > 0.0) ahead = std::min(32, std::max(3, (int)(150e-6 / t_iter) + 2));
        while (enq < max_iter && enq - k < ahead) {
            DPCG_TRY(enqueue_update());
            enq += 1;
        }
        DPCG_CHECK_LAUNCH();
        DPCG_TRY(wait_progress(prog, v, s, enq > k, tag));
    }
}

// the scalars on the host (h->scal_host) and the seconds since t0 once the stream has drained           cg.py:88 (the loop only)
static int read_scalars(dpcg_system *h, hipStream_t s, std::chrono::steady_clock::time_point t0, double *seconds) {
    DPCG_HIP(hipMemcpyAsync(h->scal_host, h->scal, sizeof(Scalars), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return DPCG_OK;
}

int hand_over_x(dpcg_system *h, double *x, hipStream_t s) {
    if (h->perm) launch_scatter_f64(h->A.n, h->perm, h->x, x, s);        // back to the caller's numbering
    else DPCG_HIP(hipMemcpyAsync(x, h->x, (size_t)h->A.n * sizeof(double), hipMemcpyDeviceToDevice, s));
    return DPCG_OK;
}

int deliver_results(dpcg_system *h, const SolveCall &c, const Scalars &sc, double seconds, bool x_in_place) {
    if (c.seconds) *c.seconds = seconds;
    if (c.iters) *c.iters = sc.k;                                                // cg.py:90
    if (c.final_res) *c.final_res = sc.res;
    if (c.res_history) DPCG_HIP(hipMemcpyAsync(c.res_history, h->hist, (size_t)(sc.k + 1) * sizeof(double), hipMemcpyDeviceToHost, c.s));
    // x is handed over in stream order: the copy is enqueued on the caller's stream, a second host sync is only
    // needed for the host-side history buffer
    if (c.x && (h->perm || !x_in_place)) DPCG_TRY(hand_over_x(h, c.x, c.s));
    if (c.res_history) DPCG_HIP(hipStreamSynchronize(c.s));
    DPCG_CHECK_LAUNCH();
    return sc.status;
}

int deliver_solve(dpcg_system *h, const SolveCall &c, std::chrono::steady_clock::time_point t0) {
    double seconds = 0.0;
    DPCG_TRY(read_scalars(h, c.s, t0, &seconds));
    DPCG_TRY(check_spin_errors(h, c.s));
    return deliver_results(h, c, *h->scal_host, seconds, false);
}

int finish_one_launch(dpcg_system *h, const SolveCall &c, std::chrono::steady_clock::time_point t0, const char *never_resident,
                      const std::function<int(const Scalars &)> &ran) {
    double seconds = 0.0;
    DPCG_TRY(read_scalars(h, c.s, t0, &seconds));
    DPCG_CHECK_LAUNCH();
    const Scalars sc = *h->scal_host;
    if (never_resident && sc.status < 0) {
        co_residency().timed_out();
        set_error(never_resident);
        return sc.status;
    }
    if (never_resident) co_residency().launched_fine();
    if (ran) DPCG_TRY(ran(sc));
    return deliver_results(h, c, sc, seconds, true);
}

namespace {
// Host side of one solve.  The GPU never waits for the host: iterations are enqueued ahead of the
// progress word that K3 posts to pinned memory, as a replayed hipGraph of `chunk` updates (launch-bound
// small systems) or update by update (large systems, where one update outlasts its three launches).
struct Solve {
    dpcg_system *h = nullptr;
    hipStream_t s = nullptr;
    int max_iter = 0, flags = 0, chunk = 8;
    const double *x_true = nullptr;
    bool use_graph = true;
    int enq = 0;             // updates enqueued so far
    bool complete = false;
    double t_iter = 0.0;     // measured seconds per update (0 = not known yet)
    bool fused = false;           // two-kernel updates (x lags one update behind until finish())
    bool defer_x = false;         // three-kernel updates with x brought up to date every second update
    bool many_launches = false;   // an update is dozens of small launches (level-scheduled SpTRSV): always replay a graph
    bool alternate = false;       // test knob DPCG_DRIVER_ALTERNATE, see enqueue_some
    unsigned calls = 0;
    std::chrono::steady_clock::time_point t0;

    volatile unsigned long long *prog() { return extras()[h].prog_host; }

    int enqueue_some() {
        // Replayed chunks for short updates (the launch overhead is what a chunk amortises) AND for long ones.  (Until round 6 updates longer
        // than 25 us were enqueued launch by launch: nothing to amortise there, it seemed -- but at 256^3 the queue idles 5.9 us between the
        // last launch of one host call and the first of the next (the K3 -> K1 gap of the traces of rounds 4-5: with or without non-temporal
        // stores), and not inside a replayed graph: 521.2 -> 516.8 us per update.  In between -- 25 .. 100 us, the 1M-row launch path, where
        // no such gap shows -- single launches stay: a chunk overshoots the converged solve by up to its length.  DPCG_GRAPH_ALWAYS=0: the old rule.)
        static const bool graph_long = [] { const char *e = getenv("DPCG_GRAPH_ALWAYS"); return !(e && e[0] == '0'); }();
        static const double long_s = [] { const char *e = getenv("DPCG_GRAPH_LONG_US"); return (e ? atof(e) : 100.0) * 1e-6; }();
        bool graph_now = use_graph && (max_iter - enq) >= chunk && (many_launches || !(t_iter > 25e-6) || (graph_long && t_iter > long_s));
        // DPCG_DRIVER_ALTERNATE (tests): mix single updates and replayed chunks -- 1, 8, 1, 1, 8, ... -- which is what a
        // per-update time hovering around the 25 us threshold does to the choice above
        if (alternate) graph_now = graph_now && (calls++ % 3) != 0;
        // Deferred-x form: the captured chunk reads p_j from h->p for even j, so a replay must start at an even update;
        // after an odd number of single updates one more single update restores the parity.
        if (graph_now && defer_x && (enq & 1)) graph_now = false;
        if (graph_now) {
            DPCG_HIP(hipGraphLaunch(h->graph_exec, s));
            enq += chunk;
        } else {
            DPCG_TRY(enqueue_iteration(h, flags, x_true, s, enq));
            enq += 1;
        }
        return DPCG_OK;
    }

    // how many updates to keep enqueued beyond the last one the GPU reported
    int run_ahead() const {
        if (t_iter <= 0.0) return 2 * chunk;
        const double cover = 150e-6;  // host launch + scheduling latency to hide
        int it = (int)(cover / t_iter) + 2;
        if (t_iter > 25e-6 && !(many_launches && use_graph)) return it < 3 ? 3 : it;
        const int chunks = (it + chunk - 1) / chunk + 1;
        return chunks * chunk;
    }

    // Enqueue the start of the solve (cg.py:58-67); the timer starts after the initial residual /
    // preconditioner work has drained, as the reference's does (cg.py:69).
    int start(dpcg_system *handle, const SolveCall &c) {
        h = handle;
        s = c.s;
        max_iter = c.max_iter;
        flags = c.flags;
        chunk = default_chunk();
        x_true = c.x_true;
        const int64_t n = h->A.n;
        const bool f32 = (flags & DPCG_SPMV_F32) != 0;
        const double *b = nullptr;
        DPCG_TRY(stage_call(h, c.b, c.x0, max_iter, f32, x_true != nullptr, s, &b));
        if (h->perm && x_true) {           // x_true arrives in the caller's numbering too
            if (!h->pxt) DPCG_TRY(dev_alloc(&h->pxt, n));
            launch_gather_f64(n, h->perm, x_true, h->pxt, s);
            x_true = h->pxt;
        }
        if ((flags & DPCG_VAL32_IF_LOSSLESS) && h->A.val32_lossless == 0) {   // decide once per matrix
            int *d_lossy = nullptr, lossy = 0;
            DPCG_TRY(dev_alloc(&d_lossy, 1));
            if (!h->A.val32) DPCG_TRY(dev_alloc(&h->A.val32, h->A.nnz));
            DPCG_HIP(hipMemsetAsync(d_lossy, 0, sizeof(int), s));
            launch_val32_check(h->A.nnz, h->A.val, h->A.val32, d_lossy, s);
            DPCG_HIP(hipMemcpyAsync(&lossy, d_lossy, sizeof(int), hipMemcpyDeviceToHost, s));
            DPCG_HIP(hipStreamSynchronize(s));
            dev_free(d_lossy);
            h->A.val32_lossless = lossy ? -1 : 1;
        }
        fused = fuse_eligible(h, flags, x_true);
        defer_x = defer_x_eligible(h, flags, x_true);
        {
            const char *e = getenv("DPCG_DRIVER_ALTERNATE");   // read per solve: tests switch it on and off
            alternate = e && e[0] == '1';
        }
        if ((fused || defer_x) && !h->p2) {
            DPCG_TRY(dev_alloc(&h->p2, n));
            drop_graph(h);
        }
        const int per_update = 3 + precond_launches(h);
        many_launches = per_update >= 16;
        if (many_launches) chunk = std::max(1, std::min(chunk, 1024 / per_update));   // keep the graph at ~1K nodes
        // a V-cycle update takes 0.1-0.3 ms at 1M rows and a multigrid solve converges in tens of updates: replayed chunks of two keep
        // the run-ahead beyond convergence short (its kernels skip once `done` is set, their launches still cost)
        if (h->precond == DPCG_PRECOND_AMG) chunk = 2;
        if (defer_x && (chunk & 1)) chunk += 1;   // a replayed chunk must start at an even update (p buffer parity)
        use_graph = !(flags & DPCG_NO_GRAPH) && !x_true && max_iter >= chunk && h->precond != DPCG_PRECOND_CALLBACK;
        if (use_graph) {
            DPCG_TRY(ensure_graph(h, flags, chunk));
            if (!h->graph_exec) use_graph = false;       // a voided capture (see ensure_graph)
        }
        double *z = h->precond == DPCG_PRECOND_NONE ? h->r : h->z;
        if (h->precond != DPCG_PRECOND_NONE) DPCG_TRY(apply_precond(h, h->r, h->z, s));   // cg.py:61
        launch_init_state(n, h->scal, b, h->r, z, h->p, f32 ? h->p32 : nullptr, h->part_bb, h->part_rz, h->part_rr,
                          (flags & DPCG_INIT_CHECK_R) ? 1 : 0, h->vec_grid, s);
        launch_finalize_init(h->scal, h->part_bb, h->part_rz, h->part_rr, h->vec_grid, c.rtol_sq, c.atol_sq, h->hist,
                             h->hist_cap, extras()[h].prog_dev, s, kMaxSpmvGrid);
        if (fused) {
            DPCG_HIP(hipMemsetAsync(h->p2, 0, (size_t)n * sizeof(double), s));       // "p_{-1}": multiplied by beta_0 = 0
            launch_fused_init(h->scal, s);
        }
        if (x_true) {                                                                // cg.py:27-29
            launch_anorm_err(n, h->scal, h->x, x_true, h->e, h->vec_grid, s);
            launch_spmv(h->A, h->planA, h->e, h->t, h->part_bb, nullptr, s);
            launch_record_err(h->scal, h->part_bb, h->planA.grid, h->err_hist, h->hist_cap, 0, s);
        }
        DPCG_CHECK_LAUNCH();
        DPCG_HIP(hipStreamSynchronize(s));
        t0 = std::chrono::steady_clock::now();                                       // cg.py:69
        if (max_iter == 0) complete = true;
        return DPCG_OK;
    }

    // Advance.  Returns a negative status on error, 1 when the solve is complete, 0 otherwise.
    int step(bool blocking) {
        if (complete) return 1;
        for (;;) {
            const unsigned long long v = *prog();
            const int k = (int)(v >> 1);
            if ((v & 1ull) || k >= max_iter) {
                complete = true;
                return 1;
            }
            if (k >= 4) t_iter = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / k;
            const int target = run_ahead();
            while (enq < max_iter && enq - k < target) DPCG_TRY(enqueue_some());
            if (!blocking) return 0;
            DPCG_TRY(wait_progress(prog(), v, s, enq > k, ""));
        }
    }

    // c: the call start() took (its x_true already stands in the member, in the handle's numbering)
    int finish(const SolveCall &c) {
        const int64_t n = h->A.n;
        if (fused)
            launch_final_fused(n, h->scal, h->part_rr, h->vec_grid, h->hist, h->hist_cap, h->x, h->p, h->p2, h->vec_grid,
                               s);
        else if (defer_x)
            launch_final_deferred(n, h->scal, h->x, h->p, h->p2, h->vec_grid, s);
        else
            launch_final_check(h->scal, s);
        const int st = deliver_solve(h, c, t0);
        if (st >= 0 && c.err_history && x_true) {      // (the count of entries is known only now)
            DPCG_HIP(hipMemcpyAsync(c.err_history, h->err_hist, (size_t)(h->scal_host->k + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
            DPCG_HIP(hipStreamSynchronize(s));
        }
        return st;
    }
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// small systems: the whole solve in one launch, one workgroup per system (dpcg_small.hip)
// ------------------------------------------------------------------------------------------------
static bool small_eligible(const dpcg_system *h, int flags, const double *x_true) {
    static const bool enabled = [] { const char *e = getenv("DPCG_SMALL"); return !(e && e[0] == '0'); }();
    if (!enabled || x_true || (flags & (DPCG_SPMV_F32 | DPCG_NO_SMALL))) return false;
    if (h->A.n > kSmallMaxN || h->perm) return false;
    return h->precond == DPCG_PRECOND_NONE || h->precond == DPCG_PRECOND_JACOBI || h->precond == DPCG_PRECOND_CSR ||
           h->precond == DPCG_PRECOND_LLT_MULTIPLY;
}

void free_ell(SmallEll &e) {
    dev_free(e.col);
    dev_free(e.val);
    e = SmallEll();
}

static int build_ell(const CsrDev &A, SmallEll &e, hipStream_t s) {
    if (e.col) return DPCG_OK;
    int *d_w = nullptr, w = 0;
    DPCG_TRY(dev_alloc(&d_w, 1));
    DPCG_HIP(hipMemsetAsync(d_w, 0, sizeof(int), s));
    launch_max_row_len((int)A.n, A.rowptr, d_w, s);
    DPCG_HIP(hipMemcpyAsync(&w, d_w, sizeof(int), hipMemcpyDeviceToHost, s));
    DPCG_HIP(hipStreamSynchronize(s));
    dev_free(d_w);
    const int64_t slabs = (A.n + 1023) / 1024;
    e.W = w < 1 ? 1 : w;
    DPCG_TRY(dev_alloc(&e.col, slabs * e.W * 1024));
    DPCG_TRY(dev_alloc(&e.val, slabs * e.W * 1024));
    launch_build_ell((int)A.n, A.rowptr, A.col, A.val, e.W, e.col, e.val, s);
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

// slab-ELL copies of the matrices the small-system kernel multiplies by (built once per matrix)
static int ensure_small(dpcg_system *h, hipStream_t s) {
    DPCG_TRY(build_ell(h->A, h->ell_a, s));
    if (h->precond == DPCG_PRECOND_CSR) DPCG_TRY(build_ell(h->M, h->ell_m, s));
    if (h->precond == DPCG_PRECOND_LLT_MULTIPLY) {
        DPCG_TRY(build_ell(h->L, h->ell_m, s));
        DPCG_TRY(build_ell(h->Lt, h->ell_t, s));
    }
    return DPCG_OK;
}

static SmallDesc make_small_desc(dpcg_system *h, const SolveCall &c) {
    SmallDesc d;
    memset(&d, 0, sizeof(d));
    d.n = (int)h->A.n;
    d.precond = h->precond;
    d.max_iter = c.max_iter;
    d.init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    d.hist_cap = h->hist_cap;
    d.lds_vectors = h->precond == DPCG_PRECOND_CSR ? 2 : (h->precond == DPCG_PRECOND_LLT_MULTIPLY ? 3 : 1);
    d.variant = small_variant((int)h->A.n, h->ell_a.W, h->precond);
    if (d.variant % 16 != 0) d.lds_vectors = 3;   // register-matrix variants: p, x and dinv live in LDS
    d.rp = h->A.rowptr; d.dinv = h->dinv;
    d.ell_a = h->ell_a; d.ell_m = h->ell_m; d.ell_t = h->ell_t;
    if (h->precond == DPCG_PRECOND_CSR) d.m_rp = h->M.rowptr;
    if (h->precond == DPCG_PRECOND_LLT_MULTIPLY) { d.m_rp = h->L.rowptr; d.t_rp = h->Lt.rowptr; }
    d.b = c.b; d.x0 = c.x0; d.x = c.x ? c.x : h->x; d.hist = h->hist;
    d.rtol_sq = c.rtol_sq; d.atol_sq = c.atol_sq;
    d.out = h->scal;
    return d;
}

static int small_variant_bit(const SmallDesc &d) { return d.variant == 4 * 16 + 7 ? 2 : (d.variant == 6 * 16 + 5 ? 4 : 1); }
static int small_lds_bytes(const SmallDesc &d) { return (int)(((size_t)d.lds_vectors * d.n + 64) * sizeof(double)); }

static int solve_small_one(dpcg_system *h, SolveCall c) {
    hipStream_t s = c.s;
    DPCG_TRY(ensure_work(h, c.max_iter, false, false));
    DPCG_TRY(ensure_small(h, s));
    if (!h->small_desc) DPCG_TRY(dev_alloc(&h->small_desc, 1));
    const SmallDesc d = make_small_desc(h, c);
    DPCG_HIP(hipMemcpyAsync(h->small_desc, &d, sizeof(d), hipMemcpyHostToDevice, s));
    DPCG_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();                                // cg.py:69 (the launch is the loop)
    DPCG_TRY(launch_pcg_small(h->small_desc, 1, small_lds_bytes(d), 1 << h->precond, small_variant_bit(d), s));
    return finish_one_launch(h, c, t0, nullptr);        // (x straight from the kernel: a reordered handle never takes this form)
}

// ------------------------------------------------------------------------------------------------
// mid-size systems: the whole solve in one launch, a team of 32 workgroups per system (dpcg_team.hip)
// ------------------------------------------------------------------------------------------------
// Rows beyond which ONE system (M = I / Jacobi) takes the team kernel instead of the one-workgroup kernel: that one holds up to 6 rows
// per thread -- 2.7 us per update at 2.4K rows, 3.0 at 4 096 (4 rows per thread), but 6.7-7.5 at 4.9K-6.1K (5-6 rows: the matrix no
// longer stays in registers) where a team takes 5.0 (tools/small_vs_team_probe.py).  Batches of such systems keep the one-workgroup
// kernel (256 of them in one launch).  DPCG_TEAM_MIN_ROWS: development knob.
static int team_min_rows() {
    static const int v = [] { const char *e = getenv("DPCG_TEAM_MIN_ROWS"); return e ? atoi(e) : 4096; }();
    return v;
}
static bool team_eligible(const dpcg_system *h, int flags, const double *x_true) {
    // eight teams of 32 workgroups, one workgroup per CU, all resident
    static const bool enabled = [] { const char *e = getenv("DPCG_TEAM"); return !(e && e[0] == '0') && device_has_cus(256); }();
    // (DPCG_VAL32_IF_LOSSLESS is a permission about how the matrix is STREAMED; the one-launch forms keep it on chip in fp64 and
    // return the same bits)
    if (!enabled || x_true || (flags & (DPCG_SPMV_F32 | DPCG_NO_TEAM | DPCG_NO_FUSE))) return false;
    if (h->A.n <= team_min_rows() || h->A.n > team_max_rows() || h->perm) return false;
    if (h->planA.max_row_len < 1 || h->planA.max_row_len > team_max_row_len()) return false;   // rows live in registers
    if (h->planA.kernel == SPMV_VECTOR) return false;     // long rows: the multi-launch path's row-sharing kernel
    return h->precond == DPCG_PRECOND_NONE || h->precond == DPCG_PRECOND_JACOBI;
}

// One mid-size system, default flags: the team kernel (with the team on one XCD -- the usual placement -- 5.0-6.3 us per update up to
// 32K rows, 7.3-9.3 up to 64K, against 9.6-14.6 for the launches: profiles/r04_team_trace.txt).  DPCG_NO_SMALL ("no whole-solve
// kernel") keeps it on the launches, as it does for the one-workgroup kernel; DPCG_TEAM_SINGLE=0: development knob.
static bool single_team_default(const dpcg_system *h, int flags) {
    static const bool on = [] { const char *e = getenv("DPCG_TEAM_SINGLE"); return !(e && e[0] == '0'); }();
    (void)h;
    return on && !(flags & (DPCG_NO_SMALL | DPCG_NO_GRAPH));
}

extern "C" int dpcg_get_reduction_geometry(dpcg_handle_t h, int32_t out[16]) {
    if (!h || !out) return invalid("dpcg_get_reduction_geometry: NULL argument");
    out[0] = h->planA.grid;
    out[1] = h->planA.nrb;
    out[2] = h->planA.kernel == SPMV_TILE ? h->planA.cyclic : 0;       // 0 slabs, 1 cyclic, 2 cyclic with XCD runs inside a pass
    out[3] = h->vec_grid;
    out[4] = fuse_eligible(h, 0, nullptr) ? 1 : 0;
    out[5] = h->planA.kernel | (h->planA.kernel == SPMV_VECTOR ? h->planA.tpr << 8 : 0);      // (+ lanes per row of the CSR-vector kernel)
    // threads of the one-workgroup solve a default call takes (0: not that form)
    out[6] = small_eligible(h, 0, nullptr) ? (small_variant((int)h->A.n, h->planA.max_row_len, h->precond) % 16 != 0 ? 768 : 1024) : 0;
    out[7] = team_eligible(h, 0, nullptr) ? (single_team_default(h, 0) ? 2 : 1) : 0;      // 2: a single default solve takes that form too
    // who sums <r,z> in a multi-launch update (cg.py:82): 0 k_update_r (M = I, Jacobi), 1 k_dot_partials, 2 k_lm_finish (way out of a
    // level-major solve), 3 the SpMV that applied M (its plan in out[9..11]), 4 the colour sweeps (out[12..15]), 9 a tree the checker
    // does not restate
    int rzk = 0;
    const SpmvPlan *pm = nullptr;
    switch (h->precond) {
        case DPCG_PRECOND_NONE: case DPCG_PRECOND_JACOBI: rzk = 0; break;
        case DPCG_PRECOND_CSR: pm = &h->planM; break;
        case DPCG_PRECOND_LLT_MULTIPLY: case DPCG_PRECOND_LU_MULTIPLY: pm = &h->planL; break;
        case DPCG_PRECOND_LLT_SOLVE: case DPCG_PRECOND_LU_SOLVE:
            rzk = h->lvlU.sweep ? 9 : ((h->lvlU.level_major && h->lvlU.strips.n_strips == 0) ? 2 : 1);
            break;
        case DPCG_PRECOND_AMG: rzk = amg_rz_partials(h->amg) > 0 ? 9 : 1; break;   // (the V-cycle's last smoothing pass)
        case DPCG_PRECOND_BLOCK_LLT_SOLVE: rzk = block_ic_rz_partials(h->bic) > 0 ? 9 : 1; break;   // (one partial per block)
        default: rzk = 1; break;
    }
    out[9] = out[10] = out[11] = 0;
    if (pm) {
        rzk = 3;
        out[9] = pm->grid;
        out[10] = pm->nrb;
        out[11] = pm->kernel == SPMV_TILE ? pm->cyclic : 0;
        // lanes per row where a CSR-vector kernel applies M (bits 8-15: M or L; 16-23: L^T of an L L^T product)
        if (pm->kernel == SPMV_VECTOR) out[11] |= pm->tpr << 8;
        if ((h->precond == DPCG_PRECOND_LLT_MULTIPLY || h->precond == DPCG_PRECOND_LU_MULTIPLY) && h->planLt.kernel == SPMV_VECTOR)
            out[11] |= h->planLt.tpr << 16;
    }
    out[12] = out[13] = out[14] = out[15] = 0;
    if (rzk == 9 && h->precond == DPCG_PRECOND_LLT_SOLVE && h->lvlU.sweep && h->lvlU.n_levels <= 16) {
        // colour sweeps: <r,z> is summed launch by launch over the levels of the upper solve -- the first of them by the lower solve's
        // last launch when that one opens the upper solve (apply_precond) -- every workgroup adding its share to its slot.
        // [12] launches, [13] workgroups, [14] two bits per launch, first launch lowest: how its workgroups walk the level's row blocks
        // (0 slabs by virtual block, 1 blocks b, b + G, ..., 2 the same by virtual block), [15] 1 = the first launch is the lower solve's
        const Levels &lo = h->lvlL, &up = h->lvlU;
        const bool paired = lo.level_major && up.level_major && up.lm_from_lower && lo.sweep && lo.lm_to_upper;
        auto mode = [](const Levels &lv, int l) {
            const bool tiled = l < (int)lv.sw_max_chunks.size() && lv.sw_max_chunks[(size_t)l] > 0;
            return tiled ? (lv.sweep_cyclic ? 2 : 0) : 1;
        };
        int packed = 0;
        for (int l = 0; l < up.n_levels; ++l) packed |= ((l == 0 && paired) ? mode(lo, lo.n_levels - 1) : mode(up, l)) << (2 * l);
        rzk = 4;
        out[12] = up.n_levels;
        out[13] = up.sweep_grid;
        out[14] = packed;
        out[15] = paired ? 1 : 0;
    }
    out[8] = rzk;
    return DPCG_OK;
}

// whether the device has that many CUs (the one-launch forms put one workgroup on each, all resident): asked once per process
bool device_has_cus(int cus) {
    static const int have = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return n;
    }();
    return have >= cus;
}

std::mutex &team_launch_mutex() {
    static std::mutex *m = new std::mutex();
    return *m;
}

CoResidency &co_residency() {
    static CoResidency *c = new CoResidency();
    return *c;
}

static int ensure_team(dpcg_system *h, hipStream_t s) {
    DPCG_TRY(build_ell(h->A, h->ell_a, s));
    if (h->ell_a.W > team_max_row_len()) return invalid("team solve: a row has more than 7 entries");
    if (!h->p2) {
        DPCG_TRY(dev_alloc(&h->p2, h->A.n));
        drop_graph(h);
    }
    if (!h->team_part) DPCG_TRY(dev_alloc(&h->team_part, 4 * 2 * 32 + 8 + 16));      // (+ 8 words of phase times, DPCG_TEAM_TRACE; + 32 ints: the XCDs)
    if (!h->team_sync) DPCG_TRY(dev_alloc(&h->team_sync, 2));
    return DPCG_OK;
}

static TeamDesc make_team_desc(dpcg_system *h, const SolveCall &c) {
    TeamDesc d;
    memset(&d, 0, sizeof(d));
    d.n = (int)h->A.n;
    d.precond = h->precond;
    d.max_iter = c.max_iter;
    d.init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    d.hist_cap = h->hist_cap;
    d.W = h->ell_a.W;
    d.rp = h->A.rowptr;
    d.dinv = h->dinv;
    d.ell_col = h->ell_a.col;
    d.ell_val = h->ell_a.val;
    d.b = c.b; d.x0 = c.x0; d.x = c.x ? c.x : h->x; d.hist = h->hist;
    d.z = h->z; d.p0 = h->p; d.p1 = h->p2;
    d.rtol_sq = c.rtol_sq; d.atol_sq = c.atol_sq;
    d.out = h->scal;
    d.bar = h->team_sync;
    d.part = h->team_part;
    d.err = reinterpret_cast<int *>(h->team_sync + 1);
    d.xcc = reinterpret_cast<int *>(h->team_part + 4 * 2 * 32 + 8);
    static const bool trace = [] { const char *e = getenv("DPCG_TEAM_TRACE"); return e && e[0] == '1'; }();
    d.dbg = trace ? reinterpret_cast<unsigned long long *>(h->team_part + 4 * 2 * 32) : nullptr;
    return d;
}

static int team_slabs_per_wg(int64_t n) {
    const int64_t slabs = (n + 1023) / 1024;
    return (int)((slabs + 31) / 32);
}

static int solve_team_one(dpcg_system *h, SolveCall c) {
    hipStream_t s = c.s;
    DPCG_TRY(ensure_work(h, c.max_iter, false, false));
    DPCG_TRY(ensure_team(h, s));
    if (!h->team_desc) {
        TeamDesc *td = nullptr;
        DPCG_TRY(dev_alloc(&td, 1));
        h->team_desc = td;
    }
    const TeamDesc d = make_team_desc(h, c);
    DPCG_HIP(hipMemcpyAsync(h->team_desc, &d, sizeof(d), hipMemcpyHostToDevice, s));
    DPCG_HIP(hipMemsetAsync(h->team_sync, 0, 2 * sizeof(unsigned int), s));
    launch_fill_pending(h->team_part, 4 * 2 * 32, s);                                // every reduction slot: "not written yet"
    DPCG_HIP(hipStreamSynchronize(s));
    // one team launch at a time per process: the workgroups of a team wait for each other, and two such launches dispatched at
    // once from two host threads could each hold part of the chip waiting for the rest of it (the 20 ms bound would end that)
    std::lock_guard<std::mutex> one_team_launch(team_launch_mutex());
    const auto t0 = std::chrono::steady_clock::now();                                // cg.py:69 (the launch is the loop)
    DPCG_TRY(launch_pcg_team(static_cast<const TeamDesc *>(h->team_desc), 1, team_slabs_per_wg(h->A.n), h->ell_a.W, s, d.dbg != nullptr));
    return finish_one_launch(h, c, t0, "team solve: a workgroup waited (20 ms) for a team member that never arrived", [&](const Scalars &sc) -> int {
        if (!d.dbg || sc.k <= 0) return DPCG_OK;
        unsigned long long w[8];
        DPCG_HIP(hipMemcpy(w, d.dbg, sizeof(w), hipMemcpyDeviceToHost));
        const double us = 0.01 / sc.k;       // 100 MHz ticks -> us per update
        fprintf(stderr, "[dpcg team] %d updates, us per update on rank 0: SpMV %.2f, sum <p,Ap> %.2f (block sums %.2f, hand-off %.2f), vector update + publish %.2f, "
                "sum <r,z> %.2f (drain %.2f, block sums %.2f, hand-off %.2f), total %.2f\n", sc.k, w[0] * us, w[1] * us, w[5] * us, (w[1] - w[5]) * us, w[2] * us,
                w[3] * us, w[6] * us, w[7] * us, (w[3] - w[6] - w[7]) * us, w[4] * us);
        return DPCG_OK;
    });
}

extern "C" int dpcg_debug_occupy(int workgroups, double milliseconds, dpcg_stream_t stream) {
    if (workgroups < 1 || workgroups > 4096 || !(milliseconds > 0.0) || milliseconds > 2000.0) return invalid("dpcg_debug_occupy: bad arguments");
    DPCG_TRY(launch_occupy(workgroups, milliseconds, (hipStream_t)stream));
    DPCG_CHECK_LAUNCH();
    return DPCG_OK;
}

extern "C" int dpcg_get_last_recurrence(dpcg_handle_t h, int *recurrence) {
    if (!h || !recurrence) return invalid("dpcg_get_last_recurrence: NULL argument");
    *recurrence = h->last_recurrence;
    return DPCG_OK;
}

static int check_solve_args(dpcg_handle_t h, const double *b, int max_iter, int flags, const double *x_true,
                            double *err_history) {
    if (!h || !b) return invalid("dpcg_solve: NULL handle or b");
    if (max_iter < 0) return invalid("dpcg_solve: max_iter < 0");
    if ((x_true == nullptr) != (err_history == nullptr) && x_true == nullptr)
        return invalid("dpcg_solve: err_history needs x_true");
    if ((flags & DPCG_SPMV_F32) && x_true) return invalid("dpcg_solve: x_true tracking is fp64 only");
    if (h->precond == DPCG_PRECOND_JACOBI && !h->dinv) return DPCG_ERR_STATE;
    return DPCG_OK;
}

extern "C" int dpcg_solve(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq,
                          double atol_sq, int max_iter, int flags, dpcg_stream_t stream, int *iters,
                          double *final_res, double *seconds, double *res_history, const double *x_true,
                          double *err_history) {
    DPCG_TRY(check_solve_args(h, b, max_iter, flags, x_true, err_history));
    // refusals first: nothing of the handle has been touched when one returns
    const char *why = h->ns ? nullspace_refusal(h, flags, x_true)
                      : h->df ? deflation_refusal(h, flags, x_true)
                      : (flags & DPCG_SINGLE_REDUCTION) ? chip_sr_refusal(h, flags, x_true) : nullptr;
    if (why) return invalid(why);
    h->last_recurrence = 0;                  // (1: set by the single-reduction chip solve, dpcg_get_last_recurrence)
    h->chip_shared_known = false;            // (set by the resident standard chip solve, dpcg_get_chip_info)
    SolveCall call{b, x0, x, rtol_sq, atol_sq, max_iter, flags, (hipStream_t)stream, iters, final_res, seconds, res_history, x_true, err_history};
    // a singular system with its null space attached, deflation vectors attached: their own drivers, whatever the size
    if (h->ns) return solve_nullspace_one(h, call);
    if (h->df) return solve_deflated_one(h, call);
    const bool one_launch_open = co_residency().open();      // (false during the cool-down after repeated co-residency timeouts)
    if (flags & DPCG_SINGLE_REDUCTION) {
        if (one_launch_open) {
            const int st = solve_chip_sr_one(h, call);
            if (st != DPCG_ERR_STATE) return st;
        }
        // the workgroups never became co-resident: the launches, with the standard recurrence (dpcg_get_last_recurrence says so)
        // (DPCG_TEAM would take the standard whole-chip kernel "whatever the other flags say" and wait out a second 20 ms: cleared too)
        call.flags = flags = (flags & ~(DPCG_SINGLE_REDUCTION | DPCG_TEAM)) | DPCG_NO_SMALL;
    }
    const bool team_first = one_launch_open && team_eligible(h, flags, x_true) && ((flags & DPCG_TEAM) || single_team_default(h, flags));
    if (small_eligible(h, flags, x_true) && !team_first) return solve_small_one(h, call);
    // a single team by default (tools/team_crossover_probe.py)
    if (team_first) {
        const int st = solve_team_one(h, call);
        if (st != DPCG_ERR_STATE) return st;
        // the team never became co-resident (a plain launch assumes it): the multi-launch path below needs no such thing
    }
    // cache-sized systems on the whole chip, in this order: M = I / Jacobi, two triangular solves, L L^T multiplied.  DPCG_ERR_STATE: the
    // kernel was refused up front, the factor does not fit the form (too many levels, rows too long) or the workgroups never became
    // co-resident -- the next form, in the end the multi-launch path, which needs no such thing
    static const struct {
        bool (*eligible)(const dpcg_system *, int, const double *);
        int (*solve)(dpcg_system *, SolveCall);
    } chip_forms[] = {{chip_eligible, solve_chip_one}, {chip_trsv_shape, solve_chip_trsv_one}, {chip_llt_eligible, solve_chip_llt_one}};
    for (const auto &form : chip_forms) {
        if (!(one_launch_open && form.eligible(h, flags, x_true) && ((flags & DPCG_TEAM) || chip_default(h, flags)))) continue;
        const int st = form.solve(h, call);
        if (st != DPCG_ERR_STATE) return st;
    }
    Solve sv;
    DPCG_TRY(sv.start(h, call));
    for (;;) {
        const int r = sv.step(true);
        if (r < 0) return r;
        if (r == 1) break;
    }
    return sv.finish(call);
}

extern "C" int dpcg_solve_batch(int count, dpcg_handle_t *handles, const double *const *b, const double *const *x0,
                                double *const *x, double rtol_sq, double atol_sq, int max_iter, int flags,
                                int n_streams, int *iters, double *final_res, double *seconds, int *status) {
    if (count <= 0 || !handles || !b) return invalid("dpcg_solve_batch: bad arguments");
    if (n_streams < 1) n_streams = 1;
    if (n_streams > 8) n_streams = 8;
    if (n_streams > count) n_streams = count;
    for (int i = 0; i < count; ++i) DPCG_TRY(check_solve_args(handles[i], b[i], max_iter, flags, nullptr, nullptr));
    for (int i = 0; i < count; ++i)
        if (handles[i]->ns) return invalid("dpcg_solve_batch: a handle with a null space is solved by dpcg_solve, one at a time");
    for (int i = 0; i < count; ++i)
        if (handles[i]->df) return invalid("dpcg_solve_batch: a handle with a deflation is solved by dpcg_solve, one at a time");
    if (flags & DPCG_SINGLE_REDUCTION) {
        for (int i = 0; i < count; ++i)
            if (const char *why = chip_sr_refusal(handles[i], flags, nullptr)) return invalid(why);     // (nothing of any handle has been touched)
    }
    // every form below runs the standard recurrence; the single-reduction members set their own word (dpcg_get_last_recurrence)
    for (int i = 0; i < count; ++i) handles[i]->last_recurrence = 0;
    for (int i = 0; i < count; ++i) handles[i]->chip_shared_known = false;
    // member i as one call on s, its scalar results into o; and the writer of a member's results, which every form below ends in
    struct Out { int it = 0; double fr = 0.0, sec = 0.0; };
    auto member = [&](int i, hipStream_t s, Out &o) {
        return SolveCall{b[i], x0 ? x0[i] : nullptr, x ? x[i] : nullptr, rtol_sq, atol_sq, max_iter, flags, s, &o.it, &o.fr, &o.sec, nullptr};
    };
    int worst = DPCG_OK;
    auto record = [&](int i, int it, double fr, double sec, int st) {
        if (iters) iters[i] = it;
        if (final_res) final_res[i] = fr;
        if (seconds) seconds[i] = sec;
        if (status) status[i] = st;
        worst = std::max(worst, st);
    };
    if (flags & DPCG_SINGLE_REDUCTION) {
        // the flag holds for every system as it does for a single solve: refused when one is not eligible, else one whole-chip launch
        // after the other (a member that cannot become co-resident goes through the launches with the standard recurrence)
        for (int i = 0; i < count; ++i) {
            Out o;
            const SolveCall c = member(i, nullptr, o);
            const int st = dpcg_solve(handles[i], c.b, c.x0, c.x, rtol_sq, atol_sq, max_iter, flags, nullptr, &o.it, &o.fr, &o.sec, nullptr, nullptr, nullptr);
            if (st < 0) return st;
            record(i, o.it, o.fr, o.sec, st);
        }
        DPCG_HIP(hipStreamSynchronize(nullptr));
        return worst;
    }
    {   // a handle owns ONE set of work vectors: the same handle twice would share them across streams
        std::vector<dpcg_handle_t> sorted(handles, handles + count);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return invalid("dpcg_solve_batch: the handles must be distinct (create one handle per system in flight)");
    }
    bool all_small = true;
    for (int i = 0; i < count; ++i) all_small = all_small && small_eligible(handles[i], flags, nullptr);
    if (all_small) {
        // one launch, one workgroup (one CU) per system
        std::vector<SmallDesc> descs((size_t)count);
        int lds = 0, kinds = 0, variants = 0;
        Out unused;
        for (int i = 0; i < count; ++i) {
            kinds |= 1 << handles[i]->precond;
            DPCG_TRY(ensure_work(handles[i], max_iter, false, false));
            DPCG_TRY(ensure_small(handles[i], nullptr));
            descs[i] = make_small_desc(handles[i], member(i, nullptr, unused));
            lds = std::max(lds, small_lds_bytes(descs[i]));
            variants |= small_variant_bit(descs[i]);
        }
        // descriptor / result arrays live across calls (hipMalloc + hipFree cost ~0.1 ms each: as much as the launch)
        struct BatchScratch {
            SmallDesc *descs = nullptr;
            Scalars *out = nullptr;
            int cap = 0;
            ~BatchScratch() {          // (allocated through the block cache: freed through it)
                dev_free(descs);
                dev_free(out);
            }
        };
        static thread_local BatchScratch scratch;
        if (scratch.cap < count) {
            dev_free(scratch.descs);
            dev_free(scratch.out);
            scratch.cap = 0;
            DPCG_TRY(dev_alloc(&scratch.descs, count));
            DPCG_TRY(dev_alloc(&scratch.out, count));
            scratch.cap = count;
        }
        SmallDesc *d_descs = scratch.descs;
        Scalars *d_out = scratch.out;        // one contiguous result array: a single copy back for the whole batch
        std::vector<Scalars> out((size_t)count);
        for (int i = 0; i < count; ++i) descs[i].out = d_out + i;
        hipError_t e = hipMemcpy(d_descs, descs.data(), descs.size() * sizeof(SmallDesc), hipMemcpyHostToDevice);
        const auto t0 = std::chrono::steady_clock::now();
        int st = e == hipSuccess ? launch_pcg_small(d_descs, count, lds, kinds, variants, nullptr) : DPCG_ERR_HIP;
        if (e == hipSuccess) e = hipMemcpy(out.data(), d_out, out.size() * sizeof(Scalars), hipMemcpyDeviceToHost);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        DPCG_HIP(e);
        if (st < 0) return st;
        for (int i = 0; i < count; ++i) record(i, out[i].k, out[i].res, sec, out[i].status);      // (sec: the batch ran as one launch)
        return worst;
    }
    bool all_chip = true;
    for (int i = 0; i < count; ++i) all_chip = all_chip && chip_eligible(handles[i], flags, nullptr);
    if (all_chip && co_residency().open() && ((flags & DPCG_TEAM) || chip_default(handles[0], flags))) {
        // cache-sized systems: the whole chip serves one system at a time (7-13 us per update against 30 for the launches -- nothing to
        // interleave), and a batch member's result is bit for bit that of its single solve
        bool refused = false;
        for (int i = 0; i < count && !refused; ++i) {
            Out o;
            const int st = solve_chip_one(handles[i], member(i, nullptr, o));
            if (st == DPCG_ERR_STATE) { refused = true; break; }     // never co-resident: the whole batch takes the streams below
            if (st < 0) return st;
            record(i, o.it, o.fr, o.sec, st);
        }
        if (!refused) {
            DPCG_HIP(hipStreamSynchronize(nullptr));
            return worst;
        }
        worst = DPCG_OK;                   // (every member is solved again)
    }
    bool all_team = true;
    for (int i = 0; i < count; ++i) all_team = all_team && team_eligible(handles[i], flags, nullptr);
    if (all_team && co_residency().open() && ((flags & DPCG_TEAM) || single_team_default(handles[0], flags))) {      // (any count: one team already beats the launches)
        // up to eight systems per launch, one team (normally: one XCD) each; the launches follow one another
        struct TeamScratch {
            TeamDesc *descs = nullptr;
            ~TeamScratch() { dev_free(descs); }
        };
        static thread_local TeamScratch scratch;
        if (!scratch.descs) DPCG_TRY(dev_alloc(&scratch.descs, 8));
        Out unused;
        bool team_timed_out = false;       // a team waited in vain for its members (the chip shared with another process, a long kernel
                                           // holding CUs: the launch is a plain one, co-residency is assumed, not guaranteed)
        for (int g0 = 0; g0 < count && !team_timed_out; g0 += 8) {
            const int ng = std::min(8, count - g0);
            TeamDesc descs[8];
            int slabs = 1, wmax = 1;
            for (int i = 0; i < ng; ++i) {
                dpcg_system *hi = handles[g0 + i];
                DPCG_TRY(ensure_work(hi, max_iter, false, false));
                DPCG_TRY(ensure_team(hi, nullptr));
                descs[i] = make_team_desc(hi, member(g0 + i, nullptr, unused));
                DPCG_HIP(hipMemsetAsync(hi->team_sync, 0, 2 * sizeof(unsigned int), nullptr));
                launch_fill_pending(hi->team_part, 4 * 2 * 32, nullptr);
                slabs = std::max(slabs, team_slabs_per_wg(hi->A.n));
                wmax = std::max(wmax, hi->ell_a.W);
            }
            DPCG_HIP(hipMemcpy(scratch.descs, descs, (size_t)ng * sizeof(TeamDesc), hipMemcpyHostToDevice));
            std::lock_guard<std::mutex> one_team_launch(team_launch_mutex());        // (see solve_team_one)
            const auto t0 = std::chrono::steady_clock::now();
            DPCG_TRY(launch_pcg_team(scratch.descs, ng, slabs, wmax, nullptr));
            DPCG_HIP(hipStreamSynchronize(nullptr));
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            DPCG_CHECK_LAUNCH();
            for (int i = 0; i < ng; ++i) {
                dpcg_system *hi = handles[g0 + i];
                DPCG_HIP(hipMemcpy(hi->scal_host, hi->scal, sizeof(Scalars), hipMemcpyDeviceToHost));
                const Scalars sc = *hi->scal_host;
                if (sc.status < 0) {
                    team_timed_out = true;
                    co_residency().timed_out();
                    break;
                }
                record(g0 + i, sc.k, sc.res, sec, sc.status);      // (sec: the group ran as one launch)
            }
        }
        if (!team_timed_out) return worst;
        worst = DPCG_OK;
        // not an error: the whole batch runs again through the multi-launch path below, which needs no co-residency
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "[dpcg] team solve: a workgroup waited 20 ms for a team member that never became resident; "
                            "the batch is solved through the multi-launch path instead\n");
    }
    StreamSet streams;                       // (synchronised and destroyed on every way out)
    DPCG_TRY(streams.create(n_streams));
    std::vector<Solve> sv((size_t)count);
    std::vector<int> slot_owner((size_t)n_streams, -1);
    int next = 0, done = 0, err = 0;
    while (done < count && !err) {
        bool progressed = false;
        for (int sl = 0; sl < n_streams && !err; ++sl) {
            int i = slot_owner[sl];
            if (i < 0) {
                if (next >= count) continue;
                i = next++;
                slot_owner[sl] = i;
                Out unused;
                const int st = sv[i].start(handles[i], member(i, streams.s[(size_t)sl], unused));
                if (st < 0) { err = st; break; }
                progressed = true;
            }
            Solve &v = sv[i];
            const int r = v.step(false);
            if (r < 0) { err = r; break; }
            if (r == 1) {
                Out o;
                const int st = v.finish(member(i, v.s, o));
                if (st < 0) { err = st; break; }
                record(i, o.it, o.fr, o.sec, st);
                slot_owner[sl] = -1;
                ++done;
                progressed = true;
            }
        }
        if (!progressed) std::this_thread::yield();
    }
    return err ? err : worst;
}
