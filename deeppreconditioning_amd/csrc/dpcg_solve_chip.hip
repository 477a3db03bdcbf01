// Host side of libdpcg.so, part 4: the whole-chip one-launch solves -- which systems take them, the plan of the triangular-solve form,
// ONE host path for the four forms (dpcg_chip.hip, dpcg_chip_sr.hip, dpcg_chip_llt.hip, dpcg_chip_trsv.hip: a form adds its descriptor, its
// launch and what it does after a launch that ran), and what the library reports of them.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>

#include "dpcg_host.h"
#include "dpcg_prims.h"

// ------------------------------------------------------------------------------------------------
// cache-sized systems: the whole solve in one launch, the whole chip as one team (dpcg_chip.hip)
// ------------------------------------------------------------------------------------------------
// 65 537 .. 1 048 576 rows, M = I / Jacobi; rows of <= 7 entries (9 up to 524 288 rows), half-bandwidth < 32 768 (stencils; meshes after the
// library's RCM): matrix and vectors resident -- otherwise, rows of up to 24 entries: the vectors resident, the matrix streamed;
// matrix and vectors stay in registers and LDS for the whole solve.  DPCG_CHIP=0 / DPCG_CHIP_MIN_ROWS: development knobs.
// the resident form: every row in the slots of its thread, every column within the 16-bit reach of its row
static bool chip_resident_shape(const dpcg_system *h, bool f32_slots = false) {
    return h->planA.max_row_len >= 1 && h->planA.max_row_len <= chip_max_row_len(h->A.n, f32_slots) && h->planA.max_band >= 0 &&
           h->planA.max_band <= chip_max_band();
}
static bool chip_enabled() {          // one workgroup per CU, all resident
    static const bool on = [] { const char *e = getenv("DPCG_CHIP"); return !(e && e[0] == '0') && device_has_cus(chip_workgroups()); }();
    return on;
}
bool chip_eligible(const dpcg_system *h, int flags, const double *x_true) {
    static const int min_rows = [] { const char *e = getenv("DPCG_CHIP_MIN_ROWS"); return e ? atoi(e) : team_max_rows(); }();
    // (DPCG_SPMV_F32: with x0 = 0, see the callers; DPCG_VAL32_IF_LOSSLESS: a permission about how the matrix is streamed -- resident in
    // fp64 the results are the same bits, so the flag does not keep a system off the chip)
    if (!chip_enabled() || x_true || (flags & (DPCG_NO_TEAM | DPCG_NO_FUSE))) return false;
    if (h->A.n <= min_rows || h->A.n > chip_max_rows()) return false;
    if (h->planA.max_row_len < 1 || h->planA.max_band < 0) return false;
    if (h->precond != DPCG_PRECOND_NONE && h->precond != DPCG_PRECOND_JACOBI) return false;
    if (chip_resident_shape(h)) return true;
    // rows too long or columns too far for the resident form: the same kernel with the matrix streamed (dpcg_chip.hip MODE 5) -- fp64,
    // rows of up to 24 entries.  Measured against the launches, us per update (profiles/r05_chip_stream_probe.txt): 1M-row quadtree meshes
    // (rows of up to 9) 21.0-22.1 / 28.8-28.9, Delaunay graphs (rows of up to 21) of 1M rows 25.5 / 31.3, 500K 14.3 / 21.7, 250K 8.9 / 17.9,
    // 100K 6.8 / 12.6.  DPCG_CHIP_STREAM=0: never (development)
    const char *e = getenv("DPCG_CHIP_STREAM");
    if (e && e[0] == '0') return false;
    return h->planA.max_row_len <= chip_stream_max_row_len();
}
// a plain call takes it (DPCG_NO_SMALL = "no whole-solve kernel for one system" keeps the launches, as for the other two)
bool chip_default(const dpcg_system *h, int flags) {
    (void)h;
    return !(flags & (DPCG_NO_SMALL | DPCG_NO_GRAPH));
}
static int chip_rows_per_wg(int64_t n) { return (int)((n + chip_workgroups() - 1) / chip_workgroups()); }

// DPCG_SINGLE_REDUCTION: the single-reduction recurrence in the whole-chip kernel (dpcg_chip_sr.hip) -- opt-in, and only where the resident
// fp64 form of the chip kernel is taken.  Why a system with the flag set cannot take it (nullptr: it can): the caller is told, the
// other recurrence is never substituted silently.
const char *chip_sr_refusal(const dpcg_system *h, int flags, const double *x_true) {
    if (x_true) return "the single-reduction recurrence does not track x_true";
    if (flags & DPCG_SPMV_F32) return "the single-reduction recurrence is fp64 only (DPCG_SPMV_F32 is set)";
    if (flags & (DPCG_NO_SMALL | DPCG_NO_GRAPH | DPCG_NO_TEAM | DPCG_NO_FUSE))
        return "the single-reduction recurrence exists in the whole-chip kernel only (DPCG_NO_SMALL / DPCG_NO_GRAPH / DPCG_NO_TEAM / DPCG_NO_FUSE keep the launches)";
    if (h->precond != DPCG_PRECOND_NONE && h->precond != DPCG_PRECOND_JACOBI)
        return "the single-reduction recurrence takes M = I or Jacobi only";
    if (h->A.n > chip_max_rows()) return "the single-reduction recurrence takes at most 1 048 576 rows";
    if (!chip_eligible(h, flags, x_true)) return "the single-reduction recurrence needs a system of the whole-chip kernel's size (more than 65 536 rows, one workgroup per CU)";
    if (h->planA.max_band > chip_max_band()) return "the single-reduction recurrence needs every column within 32 767 of its row";
    if (h->planA.max_row_len > chip_sr_max_row_len(h->A.n))
        return h->A.n > chip_max_rows() / 2 ? "the single-reduction recurrence takes rows of at most 5 entries beyond 524 288 rows"
                                            : "the single-reduction recurrence takes rows of at most 7 entries";
    return nullptr;
}

// M = L L^T multiplied (the learned technique, IC multiplied) beyond the one-workgroup kernel: the whole chip, L and L^T resident
static const CsrDev &llt_l(const dpcg_system *h) { return h->perm ? h->Lp : h->L; }
static const CsrDev &llt_t(const dpcg_system *h) { return h->perm ? h->Ltp : h->Lt; }
static bool chip_llt_tagged() {       // DPCG_CHIP_LLT_SYNC=0 (development): plain vectors and a chip-wide barrier per product
    static const bool on = [] { const char *e = getenv("DPCG_CHIP_LLT_SYNC"); return !(e && e[0] == '0'); }();
    return on;
}
bool chip_llt_eligible(const dpcg_system *h, int flags, const double *x_true) {
    if (!chip_enabled() || x_true || h->precond != DPCG_PRECOND_LLT_MULTIPLY) return false;
    if (flags & (DPCG_SPMV_F32 | DPCG_NO_TEAM | DPCG_NO_FUSE)) return false;
    if (h->A.n <= kSmallMaxN || h->A.n > chip_llt_max_rows()) return false;
    if (h->planA.max_row_len < 1 || h->planA.max_row_len > 7) return false;        // (dpcg_chip_llt.hip: rows of A of <= 7 entries)
    const int ml = std::max(h->planL.max_row_len, h->planLt.max_row_len);
    if (h->planL.max_row_len < 1 || h->planLt.max_row_len < 1 || ml > chip_llt_max_row_len()) return false;
    if (ml > 8 && h->A.n > chip_llt_max_rows() / 2) return false;      // (two rows a thread of 16-entry factor rows: beyond the registers)
    const int band = std::max(h->planA.max_band, std::max(h->planL.max_band, h->planLt.max_band));
    if (h->planA.max_band < 0 || h->planL.max_band < 0 || h->planLt.max_band < 0 || band > chip_max_band()) return false;
    return true;
}

// M = (L L^T)^-1 by two triangular solves on the whole chip (dpcg_chip_trsv.hip): A resident, L and L^T streamed as per-wave block lists
// (built here once per preconditioner: dependency levels of both triangles by the sync-free analysis, then the lists in the chip kernel's
// geometry), y and z handed from level to level as self-validating granules.
static bool chip_trsv_enabled() {
    static const bool on = [] { const char *e = getenv("DPCG_CHIP_TRSV"); return !(e && e[0] == '0') && chip_enabled(); }();
    return on;
}
static int chip_trsv_min_rows() {
    // (from 1 024 rows: measured with IC(0) in multicolour order, us per update, launches -> this kernel: 1 674 rows (quadtree mesh, 4 colours)
    // 29.4 -> 14.9, 4 268 rows 32.6 -> 16.5, 10 000 rows 25.5 -> 9.1, 13 824 rows 32.3 -> 11.7 -- an update of the launches is launch-bound there)
    static const int v = [] { const char *e = getenv("DPCG_CHIP_TRSV_MIN_ROWS"); return e ? atoi(e) : 1024; }();
    return v;
}
// what can be told without the lists (they are built at the first solve)
bool chip_trsv_shape(const dpcg_system *h, int flags, const double *x_true) {
    if (!chip_trsv_enabled() || x_true || h->precond != DPCG_PRECOND_LLT_SOLVE || h->trsv_state < 0) return false;
    if (flags & (DPCG_SPMV_F32 | DPCG_NO_TEAM | DPCG_NO_FUSE)) return false;
    if (h->A.n < chip_trsv_min_rows() || h->A.n > chip_max_rows()) return false;
    if (!chip_resident_shape(h)) return false;                       // (A resident: rows of <= 7 entries, 9 up to 524 288 rows; 16-bit column offsets)
    if (h->L.nnz <= 0 || h->Lt.nnz <= 0) return false;
    return true;
}
void free_chip_trsv(dpcg_system *h) {
    free_chip_trsv_lists(h->trsv_l);
    free_chip_trsv_lists(h->trsv_u);
    dev_free(h->trsv_lv0);
    dev_free(h->trsv_diag0);
    dev_free(h->trsv_fval);
    dev_free(h->trsv_fcol);
    dev_free(h->trsv_fmeta);
    h->trsv_rpt = h->trsv_wmax = h->trsv_band = 0;
}
static int ensure_chip_trsv(dpcg_system *h, hipStream_t s) {
    if (h->trsv_state != 0) return DPCG_OK;
    const int64_t n = h->A.n;
    PhaseTimer pt(s);
    int32_t *lvl[2] = {nullptr, nullptr}, *ctl = nullptr;
    auto done = [&](int state, int code) {
        dev_free(lvl[0]); dev_free(lvl[1]); dev_free(ctl);
        if (state < 0) free_chip_trsv(h);
        h->trsv_state = state;
        return code;
    };
    int st;
    if ((st = dev_alloc(&lvl[0], n)) < 0 || (st = dev_alloc(&lvl[1], n)) < 0) return done(0, st);
    if ((st = dev_alloc(&ctl, 4)) < 0) return done(0, st);
    // factor index <-> handle index: the factor's own numbering (multicolour IC(0)) or the caller's (a reordered handle)
    const int32_t *handle_of_f = h->fmap ? h->fmap : h->iperm;
    const int32_t *f_of_handle = h->fmap ? h->fmap_inv : h->perm;
    const int per = chip_rows_per_wg(n);
    int nlev[2] = {0, 0};
    for (int upper = 0; upper < 2; ++upper) {                          // dependency levels of both triangles (sync-free analysis, dpcg_analysis.hip)
        const CsrDev &F = upper ? h->Lt : h->L;
        DPCG_HIP(hipMemsetAsync(lvl[upper], 0xff, (size_t)n * sizeof(int32_t), s));
        DPCG_HIP(hipMemsetAsync(ctl, 0, 4 * sizeof(int32_t), s));
        launch_levels_syncfree(n, F.rowptr, F.col, upper != 0, lvl[upper], reinterpret_cast<unsigned int *>(ctl), ctl + 1, s);
        if ((st = reduce_max_i32(lvl[upper], ctl + 2, n, s)) < 0) return done(0, st);
        int32_t h_ctl[4] = {0, 0, 0, 0};
        DPCG_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, s));
        DPCG_HIP(hipStreamSynchronize(s));
        if (h_ctl[1] || h_ctl[2] < 0) return done(-1, DPCG_OK);
        nlev[upper] = h_ctl[2] + 1;
        // Every level is a hand-off from one workgroup to another -- publish, become visible, be gathered: ~1.2 us inside an XCD, ~3 across
        // -- and a chain of them is all a many-level solve is: measured at 216 K / 512 K rows with IC(0) in a scattered caller's order, 17 /
        // 18 levels: 66 / 94 us per update here against 72 / 87 for the launches (whose sync-free kernels wait in the same way).  Few levels
        // (multicolour orders: 2-9) are where this form wins (2-4 x); beyond 16 (18 up to two rows a thread) the launches keep the solve (natural orders of grids: hundreds).
        // (the three development knobs of this routine are read per plan, not per process: a plan is built once per preconditioner)
        // (up to two rows a thread -- 262 144 rows -- a level is cheaper here, the level's next block being gathered ahead: 18)
        const int level_default = chip_rows_per_wg(n) <= 2 * chip_threads() ? 18 : 16;
        const int level_limit = [&] { const char *e = getenv("DPCG_CHIP_TRSV_MAX_LEVELS"); return e ? std::min(atoi(e), chip_trsv_max_levels()) : level_default; }();
        if (nlev[upper] > level_limit) return done(-1, DPCG_OK);
    }
    h->trsv_l.n_levels = nlev[0];
    h->trsv_u.n_levels = nlev[1];
    pt.mark("chip trsv: levels");
    // <= 4 rows a thread: the factor resident beside the matrix
    const bool resident_on = [] { const char *e = getenv("DPCG_CHIP_TRSV_RESIDENT"); return !(e && e[0] == '0'); }();
    const int rpt = chip_trsv_resident_rpt(per), wmax = rpt ? chip_trsv_resident_wmax(h->planA.max_row_len, rpt) : 0;
    if (resident_on && rpt && wmax) {
        int misfit = 0, band = 0;
        if ((st = build_chip_trsv_resident((int)n, per, rpt, wmax, h->L, h->Lt, lvl[0], lvl[1], f_of_handle, handle_of_f, &h->trsv_fval, &h->trsv_fcol,
                                           &h->trsv_fmeta, &misfit, &band, &h->trsv_tstride, s)) < 0)
            return done(-1, st);
        pt.mark("chip trsv: resident plan");
        if (!misfit && std::max(band, h->planA.max_band) <= chip_max_band()) {
            h->trsv_rpt = rpt;
            h->trsv_wmax = wmax;
            h->trsv_band = band;
            return done(1, DPCG_OK);
        }
        dev_free(h->trsv_fval); dev_free(h->trsv_fcol); dev_free(h->trsv_fmeta);       // (a factor with fill: the streamed form may still take it)
    }
    // Beyond 524 288 rows (8 rows a thread) the factor cannot sit beside the matrix and would be STREAMED (the block lists below).  Measured at
    // 1M rows that form loses to the launches (IC(0) in multicolour order: 66 against 58 us per update -- every dependent step of a block is a
    // memory-side round trip of ~1.2 us, and the kernel spills): it is kept for factors the resident form refuses at <= 4 rows a thread
    // (fill: a row's L and L^T parts beyond its slots) and, beyond, behind DPCG_CHIP_TRSV_STREAM=1 (development).
    const bool stream_big = [] { const char *e = getenv("DPCG_CHIP_TRSV_STREAM"); return e && e[0] == '1'; }();
    if (!rpt && !stream_big) return done(-1, DPCG_OK);
    if (!h->trsv_lv0 && (st = dev_alloc(&h->trsv_lv0, (int64_t)chip_workgroups() * chip_threads())) < 0) return done(0, st);
    if (!h->trsv_diag0 && (st = dev_alloc(&h->trsv_diag0, chip_trsv_diag_doubles())) < 0) return done(0, st);
    DPCG_HIP(hipMemsetAsync(h->trsv_lv0, 0, (size_t)chip_workgroups() * chip_threads() * sizeof(int32_t), s));
    for (int upper = 0; upper < 2; ++upper) {
        const CsrDev &F = upper ? h->Lt : h->L;
        ChipTrsvLists &out = upper ? h->trsv_u : h->trsv_l;
        if ((st = build_chip_trsv_lists((int)n, per, nlev[upper], F, lvl[upper], f_of_handle, handle_of_f, upper != 0, out, h->trsv_lv0, h->trsv_diag0, s)) < 0) return done(-1, st);
        out.n_levels = nlev[upper];
        if (out.max_row > chip_trsv_max_factor_row() || out.max_row > std::max(h->planA.max_row_len, 5) - 1 ||
            std::max(out.band, h->planA.max_band) > chip_max_band())
            return done(-1, DPCG_OK);
        pt.mark(upper ? "chip lists (L^T)" : "chip lists (L)");
    }
    return done(1, DPCG_OK);
}

// ------------------------------------------------------------------------------------------------
// the host path the four forms share
// ------------------------------------------------------------------------------------------------
// chip_part on a handle: the reduction slots, 8 trace words per workgroup (DPCG_CHIP_TRACE), the two-int error flag, the workgroups' XCD ids,
// one word per wave of the standard form (its slot-rows whose shared operands come from registers)
struct ChipPart {
    double *base;
    static int slots() { return chip_slot_doubles(); }
    static int waves() { return chip_workgroups() * chip_threads() / 64; }
    static int64_t doubles() { return slots() + 8 * 256 + 2 + 128 + waves() / 2; }
    int *shared() const { return reinterpret_cast<int *>(base + slots() + 8 * 256 + 2 + 128); }
    unsigned long long *dbg() const { return reinterpret_cast<unsigned long long *>(base + slots()); }
    int *err() const { return reinterpret_cast<int *>(base + slots() + 8 * 256); }
    int *xcc() const { return reinterpret_cast<int *>(base + slots() + 8 * 256 + 2); }
};

// Keys the self-validating granules of one launch.  One source for every form: they share chip_zp and chip_rt on a handle, so a key must be
// unique across them.  Never 0 (the L L^T form's "untagged").
static unsigned next_chip_nonce() {
    static std::atomic<unsigned> counter{0};
    unsigned nonce = 0;
    do { nonce = ++counter; } while (nonce == 0);
    return nonce;
}

static bool chip_trace_on() {
    static const bool on = [] { const char *e = getenv("DPCG_CHIP_TRACE"); return e && e[0] == '1'; }();
    return on;
}
// Which product a resident system takes.  A slot-row whose rows are all stored around a centre is ~4 % faster with same-wave operands from
// registers; one that is not pays ~6.5 % for the branch in that instantiation (100^3, measured: DESIGN section 3).  So the instantiation with
// the centred path is taken where at least 62 % of the system's (wave, slot-row) pairs are centred (6.5 / (4 + 6.5)), the packed one --
// the kernel as it was -- elsewhere.  DPCG_CHIP_SHARED=0 / =1 (development, A/B): never / always.  Unlike the other DPCG_CHIP_* switches
// it is read at every solve, so that one process can measure both; set it before the solves start, not from another thread during one.
static bool chip_shared_on(const dpcg_system *h) {
    const char *e = getenv("DPCG_CHIP_SHARED");
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return true;
    return h->planA.chip_pairs > 0 && 50ll * h->planA.chip_centred_pairs >= 31ll * h->planA.chip_pairs;
}
static bool chip_local_ok() {          // DPCG_CHIP_LOCAL=0 (development): everything written through
    static const bool on = [] { const char *e = getenv("DPCG_CHIP_LOCAL"); return !(e && e[0] == '0'); }();
    return on;
}

// what a form adds to the shared path besides its descriptor and its launch
struct ChipForm {
    const char *never_resident;    // the error of a launch whose workgroups did not all become resident
    bool events;                   // DPCG_CHIP_EVENTS=1 brackets the kernel with HIP events
    bool rt, part2;                // the form uses chip_rt / chip_part2 (the second slot set is reset with the first, and the granule table zeroed)
};

// work vectors and the buffers of the forms on the handle; b and x0 in the handle's numbering
static int chip_prepare(dpcg_system *h, SolveCall &c, const ChipForm &form) {
    const int64_t n = h->A.n;
    DPCG_TRY(ensure_work(h, c.max_iter, false, false));
    if (!h->chip_part) DPCG_TRY(dev_alloc(&h->chip_part, ChipPart::doubles()));
    if (form.part2 && !h->chip_part2) DPCG_TRY(dev_alloc(&h->chip_part2, ChipPart::slots()));
    if (!h->chip_zp) DPCG_TRY(dev_alloc(&h->chip_zp, chip_zp_doubles(n)));
    if (form.rt && !h->chip_rt) DPCG_TRY(dev_alloc(&h->chip_rt, 2 * chip_zp_doubles(n)));      // two vectors of 2 x (n + pad) granules
    DPCG_TRY(gather_rhs(h, c.b, c.s));
    if (h->perm && c.x0) {                 // (x0 arrives in the caller's numbering too; the kernel reads it, h->x is what it writes)
        launch_gather_f64(n, h->perm, c.x0, h->t, c.s);
        c.x0 = h->t;
    }
    return DPCG_OK;
}

// the fields every descriptor names alike (ChipDesc, ChipSrDesc::c, ChipLltDesc, ChipTrsvDesc), after chip_prepare
template <typename D>
static void fill_common(D &d, dpcg_system *h, const SolveCall &c) {
    const ChipPart part{h->chip_part};
    d.n = (int)h->A.n;
    d.max_iter = c.max_iter;
    d.init_check_r = (c.flags & DPCG_INIT_CHECK_R) ? 1 : 0;
    d.hist_cap = h->hist_cap;
    d.per = chip_rows_per_wg(h->A.n);
    d.rp = h->A.rowptr; d.ci = h->A.col; d.val = h->A.val;
    d.b = c.b; d.x0 = c.x0;
    d.x = (c.x && !h->perm) ? c.x : h->x;
    d.hist = h->hist;
    d.zp = h->chip_zp;
    d.rtol_sq = c.rtol_sq; d.atol_sq = c.atol_sq;
    d.out = h->scal;
    d.part = part.base;
    d.err = part.err();
    d.xcc = chip_local_ok() ? part.xcc() : nullptr;
}
// ... and what the two forms with M = I / Jacobi add
static void fill_jacobi(ChipDesc &d, const dpcg_system *h) {
    d.precond = h->precond;
    d.dinv = h->dinv;
    d.band = h->planA.max_band;
    d.rp_nnz = (int)std::min<int64_t>(h->A.nnz, 0x1fffffff);
}

// The launch and what precedes it; the end is finish_one_launch, which the one-workgroup and the team form share.  launch(check_only)
// launches the form's kernel; ran(sc, events), if any, runs after a launch whose workgroups were all resident.
static int chip_run(dpcg_system *h, const SolveCall &c, const ChipForm &form, const std::function<int(bool)> &launch,
                    const std::function<int(const Scalars &, bool)> &ran = nullptr) {
    hipStream_t s = c.s;
    const int st0 = launch(true);                                                     // refused up front when it cannot be resident
    if (st0 != DPCG_OK) return st0;
    launch_fill_pending(h->chip_part, ChipPart::slots(), s);                          // every reduction slot: "not written yet"
    if (form.part2) launch_fill_pending(h->chip_part2, ChipPart::slots(), s);
    DPCG_HIP(hipMemsetAsync(ChipPart{h->chip_part}.err(), 0, 2 * sizeof(int), s));
    // the granule table: zeros, which no key accepts (every key is odd) -- whatever an earlier solve of either recurrence left is gone
    if (form.part2) DPCG_HIP(hipMemsetAsync(h->chip_zp, 0, (size_t)chip_zp_doubles(h->A.n) * sizeof(double), s));
    DPCG_HIP(hipStreamSynchronize(s));
    // one whole-chip launch at a time per process (see solve_team_one)
    std::lock_guard<std::mutex> one_team_launch(team_launch_mutex());
    // DPCG_CHIP_EVENTS=1 (read per solve; bench.py's roofline leg): HIP events on the launch stream around the kernel
    static hipEvent_t ev[2] = {nullptr, nullptr};                                    // (one pair for every form: created and used under the mutex)
    const char *ev_env = form.events ? getenv("DPCG_CHIP_EVENTS") : nullptr;
    const bool events = ev_env && ev_env[0] == '1';
    if (events && !ev[0]) {
        DPCG_HIP(hipEventCreate(&ev[0]));
        DPCG_HIP(hipEventCreate(&ev[1]));
    }
    const auto t0 = std::chrono::steady_clock::now();                                // cg.py:69 (the launch is the loop)
    if (events) DPCG_HIP(hipEventRecord(ev[0], s));
    DPCG_TRY(launch(false));
    if (events) DPCG_HIP(hipEventRecord(ev[1], s));
    return finish_one_launch(h, c, t0, form.never_resident, [&](const Scalars &sc) -> int {
        if (events) {
            float ms = 0.0f;
            DPCG_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            h->chip_trace_x[5] = (double)ms;
        }
        return ran ? ran(sc, events) : DPCG_OK;
    });
}

// DPCG_CHIP_TRACE=1, the standard form: ticks per phase and workgroup into what dpcg_get_chip_info reports
static int read_chip_trace(dpcg_system *h, const unsigned long long *dbg, const Scalars &sc) {
    std::vector<unsigned long long> w(8 * 256);
    DPCG_HIP(hipMemcpy(w.data(), dbg, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const double us = sc.k > 0 ? 0.01 / sc.k : 0.0;       // 100 MHz ticks -> us per update
    for (int i = 0; i < 7; ++i) h->chip_trace_us[i] = w[i] * us;                 // workgroup 0
    h->chip_trace_us[7] = (double)sc.k;
    // over the 256 workgroups: the slowest and the mean SpMV phase, the slowest publish phase
    double sp_max = 0, sp_sum = 0, pb_max = 0, pb_sum = 0;
    for (int g = 0; g < 256; ++g) {
        sp_max = std::max(sp_max, w[8 * g] * us); sp_sum += w[8 * g] * us;
        pb_max = std::max(pb_max, w[8 * g + 2] * us); pb_sum += w[8 * g + 2] * us;
    }
    h->chip_trace_x[0] = sp_max; h->chip_trace_x[1] = sp_sum / 256; h->chip_trace_x[2] = pb_max; h->chip_trace_x[3] = pb_sum / 256;
    h->chip_trace_x[4] = (double)(w[7] & 1ull);
    static const bool print = [] { const char *e = getenv("DPCG_CHIP_TRACE_PRINT"); return e && e[0] == '1'; }();
    if (print && sc.k > 0) {
        fprintf(stderr, "[dpcg chip] %d updates, groups on one XCD each: %d; us per update on workgroup 0: SpMV %.2f, sum <p,Ap> %.2f (of it waiting for the slots %.2f), "
                "vector update + publish %.2f, sum <r,z> %.2f (waiting %.2f), total %.2f; SpMV phase over the workgroups: mean %.2f max %.2f; publish: mean %.2f max %.2f\n",
                sc.k, (int)(w[7] & 1ull), w[0] * us, w[1] * us, w[5] * us, w[2] * us, w[3] * us, w[6] * us, w[4] * us, sp_sum / 256, sp_max, pb_sum / 256, pb_max);
        if (getenv("DPCG_CHIP_TRACE_ALL")) {
            for (int g = 0; g < 256; ++g) fprintf(stderr, "%s%.1f/%.1f", g % 32 ? " " : "\n   ", w[8 * g] * us, w[8 * g + 2] * us);
            fprintf(stderr, "\n");
        }
    }
    return DPCG_OK;
}

int solve_chip_one(dpcg_system *h, SolveCall c) {
    const ChipForm form{"chip solve: a workgroup waited (20 ms) for one that never became resident", /*events*/ true, /*rt*/ false, /*part2*/ false};
    DPCG_TRY(chip_prepare(h, c, form));
    ChipDesc d;
    memset(&d, 0, sizeof(d));
    fill_common(d, h, c);
    fill_jacobi(d, h);
    d.f32 = (c.flags & DPCG_SPMV_F32) ? 1 : 0;
    // (config 5 with x0 = 0 stores the values as fp32: twice the slots -- rows of 9 entries resident at any size)
    d.stream_cap = (chip_resident_shape(h, d.f32 != 0 && !c.x0) || h->A.nnz > 0x1fffffff) ? 0 : h->planA.max_row_len * 64;     // (products of the 64 rows of a wave)
    { const char *e = getenv("DPCG_CHIP_BENCH"); d.bench = e ? atoi(e) : 0; }
    const bool trace = chip_trace_on();
    if (d.f32 && (d.bench || trace || c.x0)) return DPCG_ERR_STATE;                      // (the caller goes on with the launches)
    if (d.stream_cap > 0 && (d.bench || trace)) return DPCG_ERR_STATE;
    d.dbg = trace ? ChipPart{h->chip_part}.dbg() : nullptr;
    d.shared = chip_shared_on(h) ? 1 : 0;
    d.shared_out = d.stream_cap > 0 ? nullptr : ChipPart{h->chip_part}.shared();
    return chip_run(h, c, form, [&](bool check_only) { return launch_pcg_chip(d, h->planA.max_row_len, c.s, check_only); },
                    [&](const Scalars &sc, bool) {
                        h->chip_shared_known = d.shared_out != nullptr;
                        return d.dbg ? read_chip_trace(h, d.dbg, sc) : DPCG_OK;
                    });
}

int solve_chip_sr_one(dpcg_system *h, SolveCall c) {
    const ChipForm form{"chip solve (single reduction): a workgroup waited (20 ms) for one that never became resident", /*events*/ true, /*rt*/ false, /*part2*/ true};
    DPCG_TRY(chip_prepare(h, c, form));
    ChipSrDesc ds;
    memset(&ds, 0, sizeof(ds));
    fill_common(ds.c, h, c);
    fill_jacobi(ds.c, h);
    ds.part2 = h->chip_part2;
    ds.xwork = h->x;
    ds.nonce = next_chip_nonce();
    return chip_run(h, c, form, [&](bool check_only) { return launch_pcg_chip_sr(ds, h->planA.max_row_len, c.s, check_only); },
                    [&](const Scalars &, bool events) {
                        h->last_recurrence = 1;
                        // this kernel has no phase timing: what dpcg_get_chip_info reports of an earlier traced standard solve is not this solve's
                        for (int i = 0; i < 8; ++i) h->chip_trace_us[i] = 0.0;
                        for (int i = 0; i < 5; ++i) h->chip_trace_x[i] = 0.0;
                        if (!events) h->chip_trace_x[5] = 0.0;
                        return DPCG_OK;
                    });
}

int solve_chip_llt_one(dpcg_system *h, SolveCall c) {
    // (no HIP events around this form's kernel: DPCG_CHIP_EVENTS leaves the last figure as it was)
    const ChipForm form{"chip solve (M = L L^T): a workgroup waited (20 ms) for one that never became resident", /*events*/ false, /*rt*/ true, /*part2*/ false};
    DPCG_TRY(chip_prepare(h, c, form));
    const CsrDev &Lm = llt_l(h), &Tm = llt_t(h);
    ChipLltDesc d;
    memset(&d, 0, sizeof(d));
    fill_common(d, h, c);
    d.band = std::max(h->planA.max_band, std::max(h->planL.max_band, h->planLt.max_band));
    d.lrp = Lm.rowptr; d.lci = Lm.col; d.lval = Lm.val;
    d.trp = Tm.rowptr; d.tci = Tm.col; d.tval = Tm.val;
    d.rpub = h->chip_rt;
    d.tpub = h->chip_rt + chip_zp_doubles(h->A.n);
    // r and t = L^T r reach the neighbours as self-validating granules keyed by a per-launch nonce (DPCG_CHIP_LLT_SYNC=0, development:
    // plain vectors and a chip-wide barrier per product)
    d.nonce = chip_llt_tagged() ? next_chip_nonce() : 0;
    const int max_l = std::max(h->planL.max_row_len, h->planLt.max_row_len);
    return chip_run(h, c, form, [&](bool check_only) { return launch_pcg_chip_llt(d, h->planA.max_row_len, max_l, c.s, check_only); });
}

// DPCG_CHIP_TRACE=1, the triangular-solve form: us per update by phase of the apply, mean and slowest wave of the chip, on stderr
static int print_chip_trsv_trace(const unsigned long long *dbg, const Scalars &sc) {
    std::vector<unsigned long long> w(256 * 64);
    DPCG_HIP(hipMemcpy(w.data(), dbg, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const double us = sc.k > 0 ? 0.01 / (sc.k + 1) : 0.0;   // (the applies: one per update and the first)
    static const char *names[8] = {"L sweep+prologue", "L blocks", "L polling again", "L^T sweep+prologue", "L^T blocks", "L^T polling again", "wait behind the apply", "blocks that polled again (count per apply)"};
    fprintf(stderr, "[dpcg chip trsv] %d updates; us per apply by phase, mean over the 2048 waves / slowest wave:\n", sc.k);
    for (int ph = 0; ph < 8; ++ph) {
        double sum = 0, mx = 0;
        for (int wv = 0; wv < 2048; ++wv) {
            const double val = (double)w[(size_t)wv * 8 + ph] * (ph == 7 ? (sc.k > 0 ? 1.0 / (sc.k + 1) : 0.0) : us);
            sum += val;
            mx = std::max(mx, val);
        }
        fprintf(stderr, "    %-44s %8.2f / %8.2f\n", names[ph], sum / 2048, mx);
    }
    return DPCG_OK;
}

int solve_chip_trsv_one(dpcg_system *h, SolveCall c) {
    DPCG_TRY(ensure_chip_trsv(h, c.s));
    if (h->trsv_state != 1) return DPCG_ERR_STATE;                 // this factor keeps the launches
    const ChipForm form{"chip solve (triangular solves): a workgroup waited (20 ms) for one that never became resident", /*events*/ true, /*rt*/ true, /*part2*/ false};
    DPCG_TRY(chip_prepare(h, c, form));
    ChipTrsvDesc d;
    memset(&d, 0, sizeof(d));
    fill_common(d, h, c);
    d.band = std::max(h->planA.max_band, h->trsv_rpt ? h->trsv_band : std::max(h->trsv_l.band, h->trsv_u.band));
    d.ypub = h->chip_rt;
    d.zpub = h->chip_rt + chip_zp_doubles(h->A.n);
    d.first_l = h->trsv_l.first_blk; d.first_u = h->trsv_u.first_blk;
    d.blk_l = h->trsv_l.blk; d.blk_u = h->trsv_u.blk;
    d.val_l = h->trsv_l.val; d.val_u = h->trsv_u.val;
    d.col_l = h->trsv_l.col; d.col_u = h->trsv_u.col;
    d.nent_l = h->trsv_l.n_ent; d.nent_u = h->trsv_u.n_ent;
    d.lv0 = h->trsv_lv0; d.diag0 = h->trsv_diag0;
    d.fval = h->trsv_fval; d.fcol = h->trsv_fcol; d.fmeta = h->trsv_fmeta;
    d.nlev_l = h->trsv_l.n_levels; d.nlev_u = h->trsv_u.n_levels;
    d.tstride = h->trsv_tstride;
    d.nonce = next_chip_nonce();
    struct TraceWords {            // (released on every way out)
        unsigned long long *p = nullptr;
        ~TraceWords() { dev_free(p); }
    } dbg;
    if (chip_trace_on()) {
        DPCG_TRY(dev_alloc(&dbg.p, 256 * 64));
        d.dbg = dbg.p;
    }
    const bool resident = h->trsv_rpt != 0;
    return chip_run(h, c, form,
                    [&](bool check_only) {
                        return resident ? launch_pcg_chip_trsv_resident(d, h->trsv_rpt, h->trsv_wmax, c.s, check_only)
                                        : launch_pcg_chip_trsv(d, h->planA.max_row_len, std::max(h->trsv_l.max_row, h->trsv_u.max_row), c.s, check_only);
                    },
                    [&](const Scalars &sc, bool) { return dbg.p ? print_chip_trsv_trace(dbg.p, sc) : DPCG_OK; });
}

// ------------------------------------------------------------------------------------------------
// what the library reports of the whole-chip forms
// ------------------------------------------------------------------------------------------------
extern "C" int dpcg_debug_l2_gather(int granules_per_group, int reps, const int32_t offsets[7], int depth, int written_through, dpcg_stream_t stream,
                                    double *gbs, double *us_per_pass, int *groups_local) {
    if (!offsets || granules_per_group < 32 * chip_threads() || granules_per_group % 32 != 0 || granules_per_group > (1 << 22) || reps < 1 || reps > 100000 ||
        (depth != 2 && depth != 4) || written_through < 0 || written_through > 2)
        return invalid("dpcg_debug_l2_gather: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int kSlots = chip_slot_doubles();
    double *table = nullptr, *part = nullptr;
    int *ints = nullptr;                   // 7 offsets | err (2) | xcc (257)
    unsigned long long *ticks = nullptr;
    DPCG_TRY(dev_alloc(&table, (size_t)8 * granules_per_group * 2));
    DPCG_TRY(dev_alloc(&part, kSlots));
    DPCG_TRY(dev_alloc(&ints, 8 + 2 + 260));
    DPCG_TRY(dev_alloc(&ticks, 256 + 1));
    int st = DPCG_OK;
    std::vector<unsigned long long> w(256);
    int flags[2] = {0, 0};
    hipError_t e = hipMemsetAsync(ints, 0, (8 + 2 + 260) * sizeof(int), s);
    if (e == hipSuccess) e = hipMemcpyAsync(ints, offsets, 7 * sizeof(int), hipMemcpyHostToDevice, s);
    launch_fill_pending(part, kSlots, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> one_team_launch(team_launch_mutex());
        st = launch_l2_gather_probe(table, granules_per_group, reps, ints, depth, written_through, part, ints + 8, ints + 10, ticks,
                                    reinterpret_cast<unsigned *>(ticks + 256), s);
        if (st == DPCG_OK) e = hipStreamSynchronize(s);
    }
    if (e == hipSuccess && st == DPCG_OK) e = hipMemcpy(w.data(), ticks, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && st == DPCG_OK) e = hipMemcpy(flags, ints + 8, sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && st == DPCG_OK) e = hipMemcpy(flags + 1, ints + 10 + 256, sizeof(int), hipMemcpyDeviceToHost);
    dev_free(table); dev_free(part); dev_free(ints); dev_free(ticks);
    DPCG_HIP(e);
    if (st != DPCG_OK) return st;
    unsigned long long worst = 0;
    for (unsigned long long x : w) worst = std::max(worst, x);
    if (flags[0] || worst == 0) {
        set_error("dpcg_debug_l2_gather: the workgroups never became co-resident");
        return DPCG_ERR_STATE;
    }
    const double us = (double)worst * 0.01;                   // 100 MHz
    const double bytes = (double)reps * 256.0 * 512.0 * 8.0 * 7.0 * 16.0;
    if (gbs) *gbs = bytes / (us * 1.0e-6) / 1.0e9;
    if (us_per_pass) *us_per_pass = us / reps;
    if (groups_local) *groups_local = flags[1];
    return DPCG_OK;
}

extern "C" int dpcg_get_chip_info(dpcg_handle_t h, int32_t out[10], double trace_us[8]) {
    if (!h || !out) return invalid("dpcg_get_chip_info: NULL argument");
    if (chip_trsv_shape(h, 0, nullptr) && h->trsv_state == 0) (void)ensure_chip_trsv(h, nullptr);     // (whether the factor fits is known once its lists exist)
    const bool el = chip_eligible(h, 0, nullptr) || chip_llt_eligible(h, 0, nullptr) || (chip_trsv_shape(h, 0, nullptr) && h->trsv_state == 1);
    out[0] = el ? (chip_default(h, 0) ? 2 : 1) : 0;          // 2: a plain dpcg_solve takes the chip kernel
    out[1] = chip_workgroups();
    out[2] = chip_threads();
    out[3] = chip_rows_per_wg(h->A.n);
    out[4] = h->planA.max_row_len;
    out[5] = h->planA.max_band;
    if (trace_us)
        for (int i = 0; i < 8; ++i) trace_us[i] = h->chip_trace_us[i];
    // bit 0: the last traced chip solve kept plainly stored copies (every group on one XCD); bits 8-15: lanes that share a row in the
    // form a plain solve takes now (2: M = L L^T multiplied with 16-entry factor rows on <= 256 rows a workgroup; a row's terms of the
    // dot products then sit in the even lanes)
    const bool split = chip_llt_eligible(h, 0, nullptr) && std::max(h->planL.max_row_len, h->planLt.max_row_len) > 8 &&
                       chip_rows_per_wg(h->A.n) <= chip_threads() / 2 && chip_llt_tagged();
    out[6] = (int)h->chip_trace_x[4] | ((split ? 2 : 1) << 8);
    out[7] = (int)(h->chip_trace_x[5] * 1.0e6);             // DPCG_CHIP_EVENTS=1: the last chip kernel between HIP events on its stream, ns
    // the last solve, if it was a resident standard chip solve: (wave, slot-row) pairs whose shared operands came from registers, of those
    // with a row at all (0 of 0: no such solve yet)
    out[8] = out[9] = 0;
    if (h->chip_shared_known && h->chip_part) {
        std::vector<int32_t> w(ChipPart::waves());
        DPCG_HIP(hipMemcpy(w.data(), ChipPart{h->chip_part}.shared(), w.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t x : w) { out[8] += x & 255; out[9] += (x >> 8) & 255; }
    }
    return DPCG_OK;
}
