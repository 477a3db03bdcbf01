/*
 * dpcg.h -- C ABI of the MI355X-native preconditioned-CG solve path (libdpcg.so).
 *
 * Drop-in boundary for the hot path of jsappl/DeepPreconditioning.
 * The reference has no native interface of its own: its "operator API" is Python duck typing
 * (`A @ v`, `M @ v`, `torch.inner`) inside uibk/deep_preconditioning/cg.py.  Each entry point
 * below names the reference lines whose work it replaces.  The Python mirror of the reference
 * signatures (deeppreconditioning_amd/cg.py, utils.py) binds these symbols with ctypes; the stub
 * a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Plain pointers and sizes only; no exceptions cross the ABI; every function returns a
 *     dpcg_status (negative = error, dpcg_last_error() gives the message for this thread).
 *   - Vectors are fp64, length n, DEVICE pointers unless a parameter says "host".
 *   - CSR: int32 rowptr[n+1], int32 col[nnz] (ascending inside a row), fp64 or fp32 val[nnz].
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls enqueue on it;
 *     only dpcg_solve*, dpcg_create (host inputs) and the setup routines synchronise it.
 *   - The caller owns every buffer it passes.  The handle owns its copies/analysis data (row-block
 *     maps, level sets, transposed factor, work vectors, graph).  A handle may be used by one
 *     thread at a time.
 */
#ifndef DPCG_H
#define DPCG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dpcg_system *dpcg_handle_t;
typedef void *dpcg_stream_t; /* hipStream_t */

enum dpcg_status {
    DPCG_OK = 0,            /* converged: res < rtol_sq (cg.py:71)                                  */
    DPCG_MAX_ITER = 1,      /* max_iter updates done without meeting the test (cg.py:70)            */
    DPCG_BREAKDOWN = 2,     /* NaN/Inf in the recurrence (<Ap,p> = 0 ...); reference spins silently */
    DPCG_ERR_INVALID = -1,  /* bad argument                                                         */
    DPCG_ERR_HIP = -2,      /* a HIP runtime call failed (no device, launch failure, ...)           */
    DPCG_ERR_NOMEM = -3,    /* allocation failed                                                    */
    DPCG_ERR_PIVOT = -4,    /* IC(0): non-positive pivot                                            */
    DPCG_ERR_STATE = -5     /* call order error (e.g. solve mode without a factor)                  */
};

enum dpcg_dtype { DPCG_F64 = 0, DPCG_F32 = 1 };
enum dpcg_memspace { DPCG_DEVICE = 0, DPCG_HOST = 1 };

/* How `zk = M @ rk` (cg.py:61,81) is applied. */
enum dpcg_precond {
    DPCG_PRECOND_NONE = 0,         /* M = I                         test.py:70-72  (vanilla)        */
    DPCG_PRECOND_JACOBI = 1,       /* M = diag(1/a_ii)              test.py:74-79                   */
    DPCG_PRECOND_CSR = 2,          /* z = M r, M an explicit CSR    test.py:88,105 (M = L L^T)      */
    DPCG_PRECOND_LLT_MULTIPLY = 3, /* z = L (L^T r), same operator as test.py:102-105, never formed */
    DPCG_PRECOND_LLT_SOLVE = 4,    /* z = L^-T (L^-1 r), level-scheduled SpTRSV (north_star)        */
    DPCG_PRECOND_CALLBACK = 5,     /* z = M r by a caller-supplied function (the duck-typed `M @ rk`) */
    DPCG_PRECOND_AMG = 6,          /* z = M r by one smoothed-aggregation V-cycle  test.py:95-98 (algebraic_multigrid) */
    DPCG_PRECOND_LU_MULTIPLY = 7,  /* z = L (U r), the reference's M = L U          test.py:90-93 (incomplete_lu)       */
    DPCG_PRECOND_LU_SOLVE = 8,     /* z = U^-1 (L^-1 r), level-scheduled SpTRSVs of an L U factor                      */
    DPCG_PRECOND_BLOCK_LLT_SOLVE = 9 /* z = P^T L^-T L^-1 P r, L block diagonal: one workgroup per block (dpcg_set_precond_block_ic) */
};

/* dpcg_solve flags */
enum dpcg_solve_flags {
    DPCG_INIT_CHECK_R = 1,   /* first test on <r0,r0> (scipy cg, utils.py:66-72) instead of the
                                reference's <z0,z0> (cg.py:66)                                      */
    DPCG_SPMV_F32 = 2,       /* mixed precision: A@p with fp32 val and fp32 p, fp64 everywhere else */
    DPCG_NO_GRAPH = 4,       /* launch kernels one by one instead of replaying a hipGraph           */
    DPCG_NO_SMALL = 8,       /* no whole-solve kernel for ONE system: neither the one-workgroup kernel (<= 6144 rows) nor the team
                                kernel (4 097 .. 65 536 rows, M = I / Jacobi) -- the multi-launch path */
    DPCG_VAL32_IF_LOSSLESS = 16, /* stream the matrix values as fp32 when every value survives the round trip
                                fp64 -> fp32 -> fp64 unchanged (true for the reference's data, which is fp32
                                upcast to fp64: data_set.py:121, test.py:68): 8 instead of 12 bytes per non-zero,
                                products and sums still fp64, results bit-identical.  Ignored when lossy. */
    DPCG_NO_FUSE = 32,       /* run an update as three kernels (SpMV | r,z | x,p) instead of the default two, in
                                which the SpMV kernel also forms p = z + beta p (cg.py:83) and the deferred
                                x += alpha p (cg.py:79); same arithmetic, bit-identical results              */
    DPCG_NO_TEAM = 64,       /* do not use the one-launch whole-solve kernel for mid-size systems (6 145 .. 65 536 rows,
                                M = I or Jacobi: a team of 32 workgroups per system, up to eight systems per launch) */
    DPCG_TEAM = 128,         /* use that kernel whatever the other flags say (it serves one system and batches by default:
                                5.0-9.3 us per update against 9.6-14.6 for the launches; eight teams together 4.4x their rate) */
    DPCG_SINGLE_REDUCTION = 256  /* opt-in: the single-synchronisation recurrence of Chronopoulos and Gear (1989) in the whole-chip
                                kernel (dpcg_chip_sr.hip) -- ONE chip-wide exchange an update instead of two.  M = I or Jacobi, fp64:
                                  r0 = b - A x0; z0 = dinv o r0 (M = I: z = r); p = q = 0
                                  k = 0, 1, ...: s = A z_k; gamma = <r,z>, delta = <z,s>, rho = <r,r> summed together (the first
                                    test on <z0,z0> unless DPCG_INIT_CHECK_R); history[k] = rho / <b,b> and the test of cg.py:71;
                                    stop -> count = k;  beta = gamma / gamma_prev (beta_0 = 0);
                                    den = delta - (beta * gamma) / alpha_prev (k = 0: delta); alpha = gamma / den;
                                    p = z + beta p; q = s + beta q; x += alpha p; r -= alpha q; z = dinv o r
                                den equals <p,Ap> in exact arithmetic and, like the standard kernel's <p,Ap>, is not examined: a NaN
                                residual ends the solve with DPCG_BREAKDOWN, anything else runs to max_iter.  Count, history and
                                status keep their meaning; the bits differ from the standard recurrence's.  Taken only where the
                                resident fp64 whole-chip form is (65 537 .. 1 048 576 rows, rows of <= 7 entries -- <= 5 beyond 524 288 rows -- within 32 767
                                columns of the diagonal, no x_true, not with DPCG_SPMV_F32 / DPCG_NO_SMALL / DPCG_NO_GRAPH /
                                DPCG_NO_TEAM / DPCG_NO_FUSE): anything else is refused with DPCG_ERR_INVALID and a message that
                                names the reason.  When the workgroups cannot become co-resident the call solves through the
                                launches with the STANDARD recurrence; dpcg_get_last_recurrence says which one ran. */
};

/* ---- library ------------------------------------------------------------------------------- */
int dpcg_version(void);
const char *dpcg_status_string(int status);
const char *dpcg_last_error(void);
/* Device facts for the roofline report: CU count, HBM bytes, gcnArchName into name[name_len]. */
int dpcg_device_info(int *cu_count, int64_t *hbm_bytes, char *name, int name_len);
/* Device blocks freed by the setup routines are kept for the next setup (hipFree costs ~0.14 ms a block and a
 * preconditioner setup frees dozens; the cache is bounded by DPCG_CACHE_MB, default 1024, 0 = off).  This returns them
 * to the driver.  No reference counterpart: the reference's setups run in ilupp / scipy on the host (test.py:81-88). */
int dpcg_release_cached_memory(void);

/* ---- system handle: the operator A (test.py:61-68 / train.py:93-95 pass it dense; here CSR) -- */
/* copy = 0 with DEVICE pointers borrows the arrays (caller keeps them alive); otherwise copied. */
int dpcg_create(dpcg_handle_t *out, int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                const void *val, int val_dtype, int memspace, int copy, dpcg_stream_t stream);
int dpcg_destroy(dpcg_handle_t h);
/* Introspection (any out pointer may be NULL).  spmv_kernel: 0 gather (CSR-stream), 1 CSR-vector, 2 x-tile; +16 when
 * a default solve runs two-kernel updates (see DPCG_NO_FUSE), +32 when the x-tile kernel reads its once-read streams and
 * writes y non-temporally (streams beyond the Infinity Cache), +64 when some 256-row blocks of the x-tile plan touch too many
 * places of x for an LDS tile and gather instead, +128 when the row blocks are dealt out to the workgroups cyclically instead of
 * in slabs.  precond_nnz: nnz of M (CSR), of L, or nnz(L) + nnz(U) for an L U factor. */
int dpcg_get_info(dpcg_handle_t h, int64_t *n, int64_t *nnz, int *spmv_kernel, int *precond_kind,
                  int64_t *precond_nnz, int *n_levels_lower, int *n_levels_upper);

/* ---- bandwidth-reducing reordering (BASELINE config 3: unstructured OpenFOAM numbering) ------------------------
 * The reference hands the solver whatever numbering the mesh generator produced (generate_data.py:67-74 reads the
 * OpenFOAM dump as is); a numbering that scatters neighbours makes every x[col] of `A @ p` (cg.py:75) its own cache
 * line.  dpcg_reorder computes a reverse Cuthill-McKee order ON THE DEVICE and lets the handle iterate on P A P^T.
 * Transparent to the caller: b, x0, x, x_true, dinv, M and L keep the CALLER's numbering in every call (vectors are
 * gathered / scattered on the device, matrices permuted at setup; an IC(0) / L factor is the factor of the caller's
 * matrix, its level schedule merely relabelled).  Call it before attaching a preconditioner (an attached one is
 * dropped).  mode: DPCG_REORDER_AUTO reorders only when the system has >= 65536 rows, its SpMV plan is the gather
 * kernel (no x-tile plan) AND either the measured x-gather traffic (distinct 128-byte lines per 256-row block) exceeds
 * 4x the bytes used (reverse Cuthill-McKee), or the traffic is fine on average but some row blocks are too scattered
 * for the x-tile plan (OpenFOAM appends refined cells): then the cheap REGION-BY-REGION numbering is tried -- many
 * breadth-first searches grown at once, numbered region by region and ring by ring -- and kept when the x-tile plan
 * takes the result.  DPCG_REORDER_ALWAYS: reverse Cuthill-McKee always; DPCG_REORDER_REGIONS: region by region always.
 * *applied (may be NULL) = 1 when the handle now iterates on a reordered matrix.
 * PCG is invariant under symmetric permutation up to the order of floating-point sums: iterates agree with the
 * unpermuted solve to rounding, and to 1e-10 with the CPU reference run on P A P^T (dpcg_get_permutation). */
enum dpcg_reorder_mode { DPCG_REORDER_NONE = 0, DPCG_REORDER_AUTO = 1, DPCG_REORDER_ALWAYS = 2, DPCG_REORDER_REGIONS = 3 };
/* New values on the SAME sparsity pattern: val[nnz] in the order of the arrays dpcg_create was given (the caller's
 * promise -- only values are passed).  The reference builds a fresh tensor per sample (data_set.py / test.py:61-68);
 * the pressure systems of one mesh share their pattern, and the SpMV plan and the reordering depend on nothing else,
 * so the next system costs an upload and a value permutation instead of a create (1M-DoF unstructured system: ~21 ms
 * with reordering).  The preconditioner is dropped (it was computed from the old values): attach one again -- an IC(0)
 * in multicolour order (dpcg_set_precond_ic0_ordered) keeps what its PATTERN determined meanwhile, so attaching it again
 * only computes values (1M DoF: 0.25 ms instead of 2-3.5 ms); any other preconditioner call frees that.  A handle
 * that borrows its arrays (copy = 0) borrows `val` likewise: fp64, device, 16-byte aligned; it may be the same buffer
 * rewritten in place. */
int dpcg_update_values(dpcg_handle_t h, const void *val, int val_dtype, int memspace, dpcg_stream_t stream);
int dpcg_reorder(dpcg_handle_t h, int mode, dpcg_stream_t stream, int *applied);
/* *reordered = 0/1; perm_host (may be NULL): int32[n], perm[new] = old (row `new` of the iterated matrix is the
 * caller's row `old`); gather_ratio (may be NULL): x-gather line traffic / bytes used of the caller's matrix, as
 * measured by the last dpcg_reorder call (0 if never measured). */
int dpcg_get_permutation(dpcg_handle_t h, int *reordered, int32_t *perm_host, double *gather_ratio);

/* ---- preconditioner M (test.py:70-105) ------------------------------------------------------- */
int dpcg_set_precond_none(dpcg_handle_t h);
/* dinv = NULL: 1/diag(A) is extracted on the device (test.py:76). */
int dpcg_set_precond_jacobi(dpcg_handle_t h, const double *dinv, int memspace, dpcg_stream_t stream);
int dpcg_set_precond_csr(dpcg_handle_t h, int64_t nnz, const int32_t *rowptr, const int32_t *col, const double *val,
                         int memspace, dpcg_stream_t stream);
/* L: lower-triangular CSR, columns ascending, diagonal stored LAST in each row.
 * mode = DPCG_PRECOND_LLT_MULTIPLY or DPCG_PRECOND_LLT_SOLVE.  Builds L^T and (solve) level sets. */
int dpcg_set_precond_llt(dpcg_handle_t h, int mode, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                         const double *val, int memspace, dpcg_stream_t stream);
/* IC(0) of A (stands in for ilupp.ichol0, test.py:83), then as dpcg_set_precond_llt. */
int dpcg_set_precond_ic0(dpcg_handle_t h, int mode, dpcg_stream_t stream);
/* IC(0) in an ordering of the library's choice, applied by triangular solves.  DPCG_ORDER_CALLER is dpcg_set_precond_ic0
 * (the factor ilupp.ichol0 would return for the matrix as the caller numbered it, test.py:83).  DPCG_ORDER_MULTICOLOR factors
 * Q A Q^T with the unknowns listed colour by colour (two colours by breadth-first parity when the mesh graph is bipartite --
 * every 5- / 7-point grid -- otherwise a deterministic greedy colouring): the factor's dependency graph is then only as deep
 * as the number of colours, so the two triangular solves of an apply are a handful of wide, fully parallel sweeps instead of
 * hundreds of dependent levels.  It is a DIFFERENT preconditioner from the reference's (same algorithm, another elimination
 * order: iteration counts differ, typically +20 % against a natural ordering), offered because on this hardware it is the
 * form in which an incomplete-Cholesky apply beats Jacobi to the solution.  Caller-visible vectors keep the caller's numbering.
 * dpcg_get_factor then returns L in the factor's numbering; dpcg_get_precond_ordering gives that numbering:
 * perm_host[k] = the caller's row at factor position k (int32[n], host; identity for DPCG_ORDER_CALLER), *n_colors.  The same
 * for an ILU(0) / DILU factor in multicolour order (dpcg_set_precond_ilu0), whose factors dpcg_get_lu_factors returns. */
enum dpcg_ordering { DPCG_ORDER_CALLER = 0, DPCG_ORDER_MULTICOLOR = 1 };
int dpcg_set_precond_ic0_ordered(dpcg_handle_t h, int mode, int ordering, dpcg_stream_t stream);
int dpcg_get_precond_ordering(dpcg_handle_t h, int *n_colors, int32_t *perm_host);
/* ICT with LEVEL-1 FILL: thresholded incomplete Cholesky on a static pattern, then as dpcg_set_precond_llt.  NOT what
 * ilupp.icholt computes (that is dpcg_set_precond_icholt below: a per-column entry count, not a fill level); kept because its
 * pattern is known before the values are, so it factors level-parallel on the device at any size.  The contract
 * (oracle/oracle.py::ict) is: pattern = tril(A) plus the fill created by eliminating with original entries only
 * (fill_in >= 1; 0 = no fill); row-wise numeric phase in the operation order of IC(0); an off-diagonal entry v = acc /
 * L_jj is dropped when |v| * L_jj < threshold * ||A(j:n, j)||_1 (the rule MATLAB documents for ichol 'ict').
 * fill_in = 0, threshold = 0 reproduces dpcg_set_precond_ic0 bit for bit. */
int dpcg_set_precond_ict(dpcg_handle_t h, int mode, int fill_in, double threshold, dpcg_stream_t stream);
/* ilupp.icholt(A, add_fill_in, threshold) as ILU++ defines it -- the DEFAULT incomplete-Cholesky technique of the reference's
 * harness (test.py:81-88: `ilupp.icholt(matrix, add_fill_in=1, threshold=0.1)`; ilupp 1.0.2, uv.lock:952, wraps ILU++), then as
 * dpcg_set_precond_llt.  The published algorithm (J. Mayer, ILU++, PAMM 7 (2007); Y. Saad, ILUT(p, tau), 1994, on the lower
 * triangle): column by column, w = A[k:, k] - sum_{j<k} L_kj L[k:, j]; d = sqrt(w_k); off-diagonal candidates below
 * threshold * ||w_offdiag||_2 are dropped, of the rest the nnz(A[k+1:, k]) + add_fill_in largest are kept (ties: smaller row).
 * The ilupp binary is absent from the build image: the restatement (oracle/oracle.py::icholt) is pinned to the published
 * description, not to ilupp's output; the device factor equals the restatement bit for bit.  Limits: at most 64 kept entries
 * per row / column of L and 256 candidates per column (DPCG_ERR_INVALID beyond); a non-positive pivot is DPCG_ERR_PIVOT.
 * What of A is read: in row k only the entries at or right of the diagonal (column k of the symmetric matrix), in whatever order
 * the row stores them; entries left of the diagonal are skipped, so the lower triangle may be incomplete or absent.  The factor
 * is that of the matrix with sorted rows (a reordered handle factors the CALLER's matrix: the same bits).
 * The pattern of a column depends on the values before it, so the columns are a chain.  Three forms of the device routine walk it
 * (dpcg_get_icholt_info says which one produced the attached factor); with pool_cap = (nnz - n + 1) / 2 + n add_fill_in + 1, the
 * bound on the kept off-diagonal entries of a symmetric pattern, and W = 4 waves (DPCG_ICHOLT_WAVES = 8 | 16: development):
 *   1  the LDS pipeline: W waves of one workgroup, wave w takes the columns w, w + W, ...; the factor lives in one CU's LDS.
 *      Needs n <= 4096 (12-bit row and column fields), pool_cap < 0xff00 and
 *        bytes(n, pool_cap, W) + 64 <= 160 KiB,  bytes = 4096 + 256 (W + 8) + 14 P + 2 (P mod 2) + 18 R,
 *        P = pool_cap + 64, R = n rounded up to a multiple of 4;
 *   2  the workspace pipeline: the same pipeline with the factor in a workspace in memory (13-bit fields), for what does not fit
 *      form 1 with n <= 8192 and pool_cap < 0xff00 (W = 4 or 8);
 *   3  one wave walks every column: everything else (~3 us per row).
 * A pipeline ends early -- and form 3 factors the whole matrix again, so the caller receives the same factor or form 3's refusal --
 * on: more than 64 candidates in a column, a full row of L, a non-positive pivot, a pool that would overflow (a pattern that is
 * not symmetric makes pool_cap too small), nnz(A[k+1:, k]) + add_fill_in > 64, a missing diagonal, or after 1 s.
 * dpcg_get_icholt_info then reports form 3 and the column at which the pipeline stopped (0 for what it finds while staging A).
 * Refusals (the text names the column k; the previous preconditioner stays attached):
 *   DPCG_ERR_PIVOT    "icholt: non-positive pivot at column k" (w_k <= 0 or not a number: an indefinite matrix, a NaN, an inf
 *                     below the diagonal; an inf ON the diagonal is a pivot like any other: L_kk = inf and zeros below it);
 *   DPCG_ERR_PIVOT    "icholt: missing diagonal entry at column k";
 *   DPCG_ERR_INVALID  "icholt: nnz + add_fill_in exceeds 64 entries at column k";
 *   DPCG_ERR_INVALID  "icholt: more than 256 candidates at column k";
 *   DPCG_ERR_INVALID  "icholt: a row of L would keep more than 64 entries (reached at column k)".
 * add_fill_in >= 0; threshold >= 0 (inf included: every candidate is dropped unless the column's norm is 0; a candidate EQUAL to
 * threshold * norm is kept). */
int dpcg_set_precond_icholt(dpcg_handle_t h, int mode, int add_fill_in, double threshold, dpcg_stream_t stream);
/* out = {the form that produced the attached ICholT factor (1 LDS pipeline, 2 workspace pipeline, 3 one wave), the waves W of that
 * pipeline (0 for form 3), the column at which a pipeline attempt stopped and handed the matrix to form 3 (-1: no pipeline ran, or
 * it finished), pool_cap}.  DPCG_ERR_STATE when the attached preconditioner did not come from dpcg_set_precond_icholt. */
int dpcg_get_icholt_info(dpcg_handle_t h, int32_t out[4]);
/* ilupp.ilut(A) as Saad's dual-threshold ILUT(p, tau) -- the reference harness's `incomplete_lu` technique (test.py:90-93: the
 * factors are MULTIPLIED, M = L U: mode DPCG_PRECOND_LU_MULTIPLY; DPCG_PRECOND_LU_SOLVE applies them by triangular solves).
 * Row by row in the caller's numbering (tests/ilut_restatement.py): w = A[i, :]; tau_i = threshold * ||A[i, :]||_2; for the
 * columns k < i of w in ascending order (fill included) w_k /= U_kk, dropped when |w_k| < tau_i, else w -= w_k U[k, k+1:];
 * of the L part the nnz(A[i, :i]) + add_fill_in largest stay, of the U part those >= tau_i and of them the
 * nnz(A[i, i+1:]) + add_fill_in largest (ties: the smaller column); U_ii = w_i, L_ii = 1.  The ilupp binary is absent: the
 * factor equals the restatement bit for bit, PARITY UNPINNED against ilupp itself.  Limits: 256 positions per working row and
 * 64 kept entries per row of L and of U (DPCG_ERR_INVALID beyond); a zero or non-finite pivot is DPCG_ERR_PIVOT (the error
 * text names the row).  On failure the previous preconditioner stays.  M = L U is not symmetric: dpcg_spectrum returns
 * DPCG_BREAKDOWN for these kinds, and no one-launch form takes them.  add_fill_in >= 0, threshold >= 0. */
int dpcg_set_precond_ilut(dpcg_handle_t h, int mode, int add_fill_in, double threshold, dpcg_stream_t stream);
/* ILU(0) and DILU: the zero-fill L U factorisations, the incomplete factors OpenFOAM pairs with PBiCGStab (its DILU) and the
 * counterpart of dpcg_set_precond_ic0_ordered for matrices whose values are not symmetric.  Not in the reference.  The factors go
 * where ILUT's go (L unit lower, diagonal last; U upper, diagonal first; columns ascending) and every consumer of those kinds
 * serves them.  Contract (tests/ilu0_restatement.py; the device equals it bit for bit), on the pattern of the matrix with sorted
 * rows, rows i ascending:
 *   DPCG_ILU_ILU0  for the stored k < i ascending: l_ik = a_ik / u_kk, then for the stored (k, j), j > k ascending, where (i, j) is
 *                  stored: a_ij = a_ij - l_ik u_kj (one product, one subtraction); what is left of row i at and right of the
 *                  diagonal is row i of U.
 *   DPCG_ILU_DILU  OpenFOAM's rule: d_i = a_ii, then for the stored k < i ascending whose (k, i) is stored too: t = a_ik a_ki,
 *                  t = t / d_k, d_i = d_i - t; L = I + strict_lower(A) D^-1, U = D + strict_upper(A).  A pattern that is not
 *                  structurally symmetric is accepted (a missing (k, i) contributes nothing).  Equal to ILU(0) where the pattern
 *                  holds no triangle (5- / 7-point grids).
 * mode: DPCG_PRECOND_LU_SOLVE (z = U^-1 L^-1 r) or DPCG_PRECOND_LU_MULTIPLY (z = L (U r), as ILUT's).
 * ordering: DPCG_ORDER_CALLER factors the matrix as the caller numbered it (also on a reordered handle);
 * DPCG_ORDER_MULTICOLOR (LU_SOLVE only) factors Q A Q^T, the unknowns listed colour by colour -- the handle's colouring, shared
 * with IC(0) in that order and kept across dpcg_update_values -- so that each triangular solve is as many wide sweeps as there
 * are colours; the lower result then reaches the upper solve by position, without leaving level order.  A different
 * preconditioner from the caller-ordered one (more iterations, far shallower applies).  The factorisation itself runs level by
 * level on the level sets of L's pattern, one row per lane: the level analysis decides what waits for what, not the colouring.
 * dpcg_get_lu_factors returns the factors in the factor's numbering, dpcg_get_precond_ordering that numbering and the colours.
 * Refusals (the previous preconditioner stays attached): DPCG_ERR_PIVOT "ILU(0): missing diagonal entry"; DPCG_ERR_PIVOT
 * "ILU(0): zero or non-finite pivot at row i" (the first such row, in the factor's numbering; both variants); DPCG_ERR_INVALID
 * for a bad mode, variant or ordering, and for the multicolour ordering in multiply mode.
 * dpcg_update_values drops the factor like any other: a refresh of the values alone on the kept pattern, as IC(0) in multicolour
 * order has, is not provided.  M = L U is not symmetric: dpcg_spectrum returns DPCG_BREAKDOWN, no one-launch form takes it. */
enum dpcg_ilu_variant { DPCG_ILU_ILU0 = 0, DPCG_ILU_DILU = 1 };
int dpcg_set_precond_ilu0(dpcg_handle_t h, int mode, int variant, int ordering, dpcg_stream_t stream);
/* The attached L U factor in the factor's numbering -- the caller's, unless the factor was built in multicolour order
 * (dpcg_get_precond_ordering) -- as host arrays (any may be NULL: with all NULL only the sizes are reported):
 * L unit lower (diagonal last), U upper (diagonal first), columns ascending.  DPCG_ERR_STATE when no L U factor is set. */
int dpcg_get_lu_factors(dpcg_handle_t h, int64_t *l_nnz, int64_t *u_nnz, int32_t *l_rowptr, int32_t *l_col, double *l_val,
                        int32_t *u_rowptr, int32_t *u_col, double *u_val);
/* The factorised sparse approximate inverse (FSAI; Kolotilina & Yeremin, SIAM J. Matrix Anal. Appl. 14 (1993)): the factor that
 * is MADE to be multiplied.  P: a symmetric pattern with the diagonal; for column i, P_i = { j >= i : (j, i) in P } ascending
 * (first element i), m_i = |P_i|; A[P_i, P_i] y = e_1 (dense SPD), L[P_i, i] = y / sqrt(y_1).  Then (L^T A)[i, j] = 0 for j in
 * P_i \ {i}, (L^T A L)[i, i] = 1, and M = L L^T ~ A^-1 is SPD for every SPD A.  Not in the reference: it is the closed-form
 * optimum of || I - L^T U_A ||_F (A = U_A U_A^T) on the kind of pattern the reference's network is trained on.
 * dpcg_set_precond_fsai: P = the pattern of A^level as a structural power (level 1, 2 or 3; level 1: tril(A), as IC(0)).
 * dpcg_set_precond_fsai_pattern: tril(P) by rows from the caller (int32 CSR, values none; lower triangular, columns ascending,
 * the diagonal last in every row; memspace DPCG_HOST or DPCG_DEVICE) -- the optimum on the exact pattern a network emits.
 * The factor is attached exactly as dpcg_set_precond_llt(DPCG_PRECOND_LLT_MULTIPLY) attaches one (kind 3: dpcg_get_factor,
 * dpcg_precond_apply, dpcg_spectrum, the one-launch forms and the batch path serve it unchanged); there is no apply mode.
 * Everything happens in the CALLER's numbering (a reordered handle gives the same bits).  Operation order of a local solve
 * (tests/fsai_restatement.py; the device equals it bit for bit): only b_pq = A[P_i[p], P_i[q]], q <= p, is read (absent: 0);
 * Cholesky column by column, s = b_pj - sum_{k<j} c_pk c_jk with k ascending, c_jj = sqrt(s_j), c_pj = s_p / c_jj; C w = e_1
 * and C^T y = w column-oriented (s_p -= c_pj w_j for j ascending; s_p -= c_jp y_j for j descending; w_j, y_j = s_j / c_jj);
 * l_p = y_p / sqrt(y_0).  No tree-shaped sums.
 * Limits and errors: m_i <= 64 (beyond: DPCG_ERR_INVALID, the text names the column and its m_i); a structurally missing
 * diagonal and a level outside 1 .. 3 are DPCG_ERR_INVALID; so is a matrix with a row whose columns do not strictly ascend (the
 * solves take such rows, but the gather map is built by bisection on A's rows: both calls check every row and refuse, the text
 * says "ascending" and names the first such row -- they never return a factor of entries they failed to find); a non-positive or non-finite pivot of a local Cholesky is
 * DPCG_ERR_PIVOT (the text names the column); the gather map holds sum m_i (m_i + 1) / 2 int32 entries, at most 2^31
 * (DPCG_ERR_INVALID beyond).  On any failure the previous preconditioner stays.
 * Reuse: the pattern, the gather map and the binning by m_i stay on the handle, keyed on (level | the explicit pattern), across
 * dpcg_update_values; attaching the same key again computes only values.  They are freed when another kind of preconditioner is
 * attached (dpcg_set_precond_none / jacobi / csr / llt / ic0 / ict / icholt / ilut / amg / callback), by dpcg_reorder and by
 * dpcg_destroy; a failed attach of another FSAI key leaves them as they were. */
int dpcg_set_precond_fsai(dpcg_handle_t h, int level, dpcg_stream_t stream);
int dpcg_set_precond_fsai_pattern(dpcg_handle_t h, int64_t nnz, const int32_t *rowptr, const int32_t *col, int memspace,
                                  dpcg_stream_t stream);
/* out = {level (0: explicit pattern), max m_i, columns with m_i <= 4, 5 .. 8, 9 .. 16, 17 .. 32, 33 .. 64, 1 when the last attach
 * reused the symbolic phase}; nnz(L) is dpcg_get_info's.  DPCG_ERR_STATE when the attached preconditioner is not an FSAI factor. */
int dpcg_get_fsai_info(dpcg_handle_t h, int32_t out[8]);
/* Block-Jacobi incomplete Cholesky: the unknowns are partitioned, every block is factored on its own, couplings between blocks
 * are dropped (what OpenFOAM's DIC does per subdomain of a decomposed run and PETSc's bjacobi + icc does by default).  Not in the
 * reference.  Contract (tests/block_ic_restatement.py; the device equals it bit for bit):
 *   numbering  rows sorted stably by (block id, caller's row); perm[k] = the caller's row at factor position k; blocks = the maximal
 *              runs of equal id.  Ids are any non-negative int32, need not be dense; a block holds at most 4096 rows.
 *   A_B        P A P^T without the entries whose row and column lie in different blocks.
 *   IC(0)      DPCG_BLOCK_IC_IC0: L = oracle.ic0(A_B) -- pattern tril(A_B), rows in factor order, sums over ascending columns one
 *              product at a time, no contraction (the order of dpcg_set_precond_ic0).
 *   DIC        DPCG_BLOCK_IC_DIC: d_i = a_ii - sum a_ij a_ij / d_j over the stored j < i of row i of A_B ascending (per term one
 *              product, one division, one subtraction); L_ij = a_ij / sqrt(d_j), L_ii = sqrt(d_i).  Equal to IC(0) mathematically
 *              (not bitwise) where tril(A_B) holds no triangle (5- / 7-point grids), different on meshes with hanging nodes.
 *   apply      z = P^T L^-T L^-1 P r by substitution: row sums in the factor's CSR order, then the division (oracle.sptrsv_lower,
 *              oracle.sptrsv_upper_t).  M is SPD for every SPD A.
 * block_of_row == NULL: contiguous runs of block_rows caller rows (1 .. 4096; the last run may be shorter); otherwise n ids
 * (memspace DPCG_HOST or DPCG_DEVICE) and block_rows is ignored.
 * One launch applies M: one workgroup per block gathers its slice of r into LDS, solves L and L^T in place level by level with a
 * workgroup barrier between levels and scatters z; in the PCG loop it leaves one partial of <r, z> per block (up to 2048 blocks;
 * beyond, the dot kernel runs).  The workgroup has 64 lanes for blocks of up to 64 rows, 128 up to 512, 256 up to 2048, else 512.
 * Served by the multi-launch PCG driver (graph replay included), the null-space and deflated drivers, dpcg_precond_apply,
 * dpcg_spectrum, dpcg_guess_* and -- through the launches, as kinds 4 and 8 -- dpcg_solve_batch; no one-launch form (one workgroup,
 * team, whole chip), DPCG_SINGLE_REDUCTION, dpcg_solve_refined or dpcg_sptrsv takes it.  dpcg_get_factor returns L in the factor
 * numbering, dpcg_get_precond_ordering gives 0 colours and perm, dpcg_get_info nnz(L) (its level counts are those of other kinds:
 * see dpcg_get_block_ic_info).
 * Errors: DPCG_ERR_PIVOT for a non-positive or non-finite pivot (the text names the caller's row); DPCG_ERR_INVALID for a block of
 * more than 4096 rows (the text names the block id and its size), a negative id, a missing diagonal, a row whose columns do not
 * strictly ascend.  After any failure the previous preconditioner stays.
 * Reuse: numbering, block extraction and level sets stay on the handle across dpcg_update_values; an attach with the same ids (either
 * variant) computes only values.  dpcg_reorder keeps an attached block factor attached -- blocks and factor are the caller's, a
 * reordered handle gives the same bits -- and rebuilds its maps into the handle's vectors. */
enum dpcg_block_ic_variant { DPCG_BLOCK_IC_IC0 = 0, DPCG_BLOCK_IC_DIC = 1 };
int dpcg_set_precond_block_ic(dpcg_handle_t h, int variant, int block_rows, const int32_t *block_of_row, int memspace,
                              dpcg_stream_t stream);
/* out = {variant, blocks, rows of the largest block, most levels of L in any block, the same for L^T, the apply kernel's workgroup
 * size, 1 when the last attach reused the symbolic phase, 0}.  DPCG_ERR_STATE for any other preconditioner. */
int dpcg_get_block_ic_info(dpcg_handle_t h, int32_t out[8]);
/* The reference's operator protocol asks of M nothing but `M @ rk` (cg.py:61,81).  An M that is not a matrix this library
 * can hold (a Python object with __matmul__, a multigrid cycle, ...) is applied through a function the caller supplies:
 * fn(user, r, z, n, stream) must ENQUEUE z = M r on `stream` (device pointers, caller's numbering; it is called from the
 * thread inside dpcg_solve, once per update, and keeps being called for the few updates the driver has enqueued beyond
 * convergence).  Slow path by construction -- one host call per update, no graph replay, vectors gathered / scattered
 * around the call on a reordered handle -- while SpMV, dots and vector updates stay the HIP kernels. */
typedef void (*dpcg_precond_fn)(void *user, const double *r, double *z, int64_t n, dpcg_stream_t stream);
int dpcg_set_precond_callback(dpcg_handle_t h, dpcg_precond_fn fn, void *user);
/* Smoothed-aggregation algebraic multigrid -- the reference harness's `algebraic_multigrid` (test.py:95-98: pyamg's
 * smoothed_aggregation_solver(A).aspreconditioner(cycle="V")) -- set up on the device and applied as ONE V(sweeps, sweeps) cycle
 * per update inside the multi-launch PCG loop (graph replay included).  The hierarchy, level by level (rules that look at a row
 * index use the caller's index, so a reordered handle gets the same aggregates):
 *   strength: j is a strong neighbour of i when j != i, a_ij != 0 and |a_ij| >= theta sqrt(|a_ii a_jj|) (theta = 0: every non-zero);
 *   roots: a deterministic parallel MIS(2) on tuples (state, splitmix64(seed, index), index), OUT < UNDECIDED < IN (Bell, Dalton,
 *   Olson 2012); aggregates: a root's neighbours join it, the others the step-1-assigned neighbour of largest |a_ij| (ties: smaller
 *   index); aggregates are numbered by ascending index of their root;
 *   T = 1/sqrt(|aggregate|) per row; P = (I - omega D^-1 A) T, omega = (4/3) / rho, rho = theta_max + err_max of a 30-step Lanczos
 *   estimate of the spectrum of D^-1 A (see dpcg_spectrum; start vector from `seed`); A_c = P^T (A P) by a row-wise device SpGEMM
 *   that sums every entry in one fixed order (two setups give the same bits).
 * Coarsening stops at max_coarse rows, at max_levels or when it stalls (n_c > 0.9 n); the coarsest level is solved exactly (dense
 * inverse by Cholesky on the host, a GEMV on the device): more than 4096 rows there is DPCG_ERR_INVALID, not positive definite
 * DPCG_ERR_PIVOT; a missing, zero or negative diagonal on any level is DPCG_ERR_PIVOT.  On any failure the previous preconditioner
 * stays.  The cycle smooths with damped Jacobi (weight omega, `sweeps` sweeps before and after; pyamg's default is Gauss-Seidel,
 * which is sequential -- dpcg_set_precond_amg_smoothed offers multicolour Gauss-Seidel and Chebyshev): M is symmetric positive
 * definite.
 * Same-pattern reuse: after dpcg_update_values, attaching again with the same parameters keeps, level by level while the aggregates
 * come out unchanged, the structures of the SpGEMMs and of P^T; only values are computed again (the result equals a fresh setup bit
 * for bit; dpcg_get_amg_info's reused_levels says how many levels were taken over).  Any other preconditioner call frees what was kept.  The one-launch forms do not take this kind. */
int dpcg_set_precond_amg(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                         dpcg_stream_t stream);
/* The same hierarchy with another smoother in the cycle (dpcg_set_precond_amg = DPCG_AMG_JACOBI).  Strength, aggregates, P (still
 * the Jacobi-smoothed prolongator), the Galerkin levels and the coarse inverse do not depend on the choice; the V(sweeps, sweeps)
 * cycle keeps its shape and only the smoother differs.  Each is self-adjoint in the A inner product, so M stays SPD.
 *   DPCG_AMG_GAUSS_SEIDEL: symmetric Gauss-Seidel in multicolour order.  Level l is coloured (multicolour ordering of dpcg_reorder;
 *     level 0 reuses the handle's cached colouring); a colour pass updates every row of one colour at once,
 *     x_i += (b_i - sum_j a_ij x_j) / a_ii; a sweep is the passes 0, 1, .., m-1, m-2, .., 0 (the repeated pass m-1 is skipped: it
 *     is a no-op).  A level whose graph needs more than 63 colours keeps damped Jacobi (dpcg_get_amg_smoothers reports it).  pyamg
 *     sweeps in row order instead (sequential); this is its parallel counterpart, not the same operator.
 *   DPCG_AMG_CHEBYSHEV: Saad's Chebyshev iteration of `degree` (1 .. 8) steps with a Jacobi preconditioner on [rho_l / eig_ratio,
 *     rho_l] (rho_l: the level's Lanczos estimate of lambda_max(D^-1 A_l), eig_ratio > 1).
 * `sweeps` counts smoother applications for every kind; degree and eig_ratio are read for DPCG_AMG_CHEBYSHEV only (but still
 * checked).  Argument errors are DPCG_ERR_INVALID and leave the handle as it was.  A re-attach after dpcg_update_values reuses
 * structures (colourings included) when every parameter, smoother, degree and eig_ratio included, is the same. */
enum dpcg_amg_smoother { DPCG_AMG_JACOBI = 0, DPCG_AMG_GAUSS_SEIDEL = 1, DPCG_AMG_CHEBYSHEV = 2 };
int dpcg_set_precond_amg_smoothed(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                                  int smoother, int degree, double eig_ratio, dpcg_stream_t stream);
/* The same hierarchy and cycle with the cycle's operands and work vectors STORED in single precision (DPCG_AMG_FP64: exactly
 * dpcg_set_precond_amg_smoothed).  The V-cycle is bound by the bytes it moves, not by arithmetic; hypre, AmgX and Ginkgo offer
 * the same under a double-precision Krylov method.  PCG's own recurrences stay fp64, so the attainable accuracy does not change;
 * only M is perturbed, at the 6e-8 level.  The contract of DPCG_AMG_FP32:
 *   setup: the hierarchy is built in fp64 exactly as for DPCG_AMG_FP64 (dpcg_get_amg_info / _level return the same bits);
 *   copies: after the setup (and after every re-attach) the values of A_l, P_l, P_l^T (the rounded numbers of P_l) and dinv_l of
 *     every level but the coarsest are stored once more, rounded to fp32 (nearest even); patterns are shared; the fp64 arrays stay;
 *   coarsest level: the dense inverse stays fp64 (small, and the one operator whose rounding error kappa(A_c) amplifies); it reads
 *     the fp32 right-hand side and its result is rounded to fp32;
 *   work vectors: all fp32, except that level 0 reads PCG's r and writes z in fp64 (neither is rounded; the <r, z> partials are
 *     formed in fp64 from those values);
 *   arithmetic: fp64 throughout -- operands are converted on load, products and row sums are fp64, omega and the Chebyshev scalars
 *     are double.  Whatever the fp64 cycle stores to a work vector is rounded to fp32 where it is computed, whether it is then
 *     stored or consumed in place: the gathered y_j = omega dinv_j b_j and y_j = x_j + omega dinv_j r_j are rounded before they
 *     enter a row sum (r = b - A x is formed from exactly the x that is stored), and so are Chebyshev's d'_j and x_j + d'_j (the
 *     last step of a level stores no d', so there d' is not rounded);
 *   smoothers: DPCG_AMG_JACOBI and DPCG_AMG_CHEBYSHEV; DPCG_AMG_GAUSS_SEIDEL with DPCG_AMG_FP32 is DPCG_ERR_INVALID (its cost is
 *     its colour passes, not its bytes), as is an unknown precision; the attached preconditioner stays;
 *   launches: the same as the fp64 cycle's; no float atomics: two applies give the same bits.
 * A hierarchy parked by dpcg_update_values is taken over whatever its precision was: copies and work vectors are made anew. */
enum dpcg_amg_precision { DPCG_AMG_FP64 = 0, DPCG_AMG_FP32 = 1 };
int dpcg_set_precond_amg_precision(dpcg_handle_t h, double theta, int max_levels, int max_coarse, int sweeps, uint64_t seed,
                                   int smoother, int degree, double eig_ratio, int precision, dpcg_stream_t stream);
/* *precision: the dpcg_amg_precision of the attached hierarchy's cycle.  DPCG_ERR_STATE when the handle's preconditioner is not AMG. */
int dpcg_get_amg_precision(dpcg_handle_t h, int *precision);
/* *launches: the kernel launches of one V-cycle of the attached hierarchy; *rz_partials: the per-workgroup partials of <r, z> its
 * last smoothing pass leaves for PCG (0: PCG sums <r, z> itself).  Neither depends on the precision.  Either pointer may be NULL.
 * DPCG_ERR_STATE when the handle's preconditioner is not AMG. */
int dpcg_get_amg_launches(dpcg_handle_t h, int *launches, int *rz_partials);
/* Per smoothed level l < min(capacity, n_levels - 1) (host arrays, any may be NULL): the smoother the level USES (a Gauss-Seidel
 * level that could not be coloured reports DPCG_AMG_JACOBI), its number of colours (0 unless Gauss-Seidel) and the Chebyshev
 * interval [lower, upper] (0 unless Chebyshev).  DPCG_ERR_STATE when the handle's preconditioner is not AMG. */
int dpcg_get_amg_smoothers(dpcg_handle_t h, int capacity, int *smoother, int *n_colors, double *cheb_lower, double *cheb_upper);
/* color[n] (host): the colour of each row of smoothed level `level` (level 0 in the caller's numbering).  DPCG_ERR_INVALID when
 * level or n is not the attached hierarchy's (nothing written), DPCG_ERR_STATE when the level is not Gauss-Seidel-smoothed. */
int dpcg_get_amg_colors(dpcg_handle_t h, int level, int64_t n, int32_t *color, dpcg_stream_t stream);
/* *n_levels; per level l < capacity (host arrays, any may be NULL): rows, nnz of A_l, nnz of P_l (0 on the coarsest), rho and
 * omega (0 on the coarsest); operator complexity sum nnz(A_l) / nnz(A_0), grid complexity sum n_l / n_0; *reused_levels: how many
 * levels the setup that built this hierarchy took over from a parked one (same-pattern reuse; 0 for a fresh build).  Any out
 * pointer may be NULL.  DPCG_ERR_STATE when the handle's preconditioner is not this kind. */
int dpcg_get_amg_info(dpcg_handle_t h, int capacity, int *n_levels, int64_t *rows, int64_t *nnz, int64_t *p_nnz, double *rho,
                      double *omega, double *operator_complexity, double *grid_complexity, int *reused_levels);
/* Host copies of level l (0 <= l < n_levels - 1), any pointer may be NULL: agg[n_l] (the aggregate of each row; level 0 in the
 * caller's numbering), P_l (n_l x n_{l+1} CSR; level 0's rows in the caller's numbering) and A_{l+1}.  sizes = {n_l, nnz(P_l),
 * n_{l+1}, nnz(A_{l+1})}, the sizes the caller's buffers were made for (from dpcg_get_amg_info): when they are not the attached
 * hierarchy's -- it was rebuilt meanwhile -- nothing is written and the call returns DPCG_ERR_INVALID.  Copies on `stream`, which
 * is synchronised. */
int dpcg_get_amg_level(dpcg_handle_t h, int level, const int64_t sizes[4], int32_t *agg, int32_t *p_rowptr, int32_t *p_col,
                       double *p_val, int32_t *a_rowptr, int32_t *a_col, double *a_val, dpcg_stream_t stream);
/* The geometry of the handle's reductions, for a checker that wants to sum in the same order (oracle/pcg_oracle.c,
 * orc_set_dot_tree: with it the CPU restatement reproduces the multi-launch solve's residual history BIT FOR BIT for M = I /
 * Jacobi): out[0] = workgroups of the SpMV kernel of the PCG loop, out[1] = its 256-row blocks, out[2] = 1 when the blocks are
 * dealt out cyclically, 2 when cyclically with an XCD's blocks of a pass contiguous (0: contiguous slabs), out[3] = workgroups of the vector kernels, out[4] = 1 when a solve with default
 * flags runs two-kernel updates, out[5] = the SpMV kernel in bits 0-7 (0 gather, 1 vector, 2 x-tile) and, for the vector kernel, its
 * lanes per row in bits 8-15, out[6] = threads of the one-workgroup
 * solve when a default call takes that form (0 otherwise), out[7] = 1 when the system is eligible for the team solve (2: and a
 * single default solve takes it),
 * out[8] = who sums <r,z> behind the CURRENT preconditioner in a multi-launch update (0 the r-update kernel, 1 a separate dot
 * launch, 2 the way-out pass of a level-major triangular solve, 3 the SpMV that applied M -- its grid / row blocks / walk in
 * out[9..11]; out[11] bits 8-15: lanes per row when that SpMV is the vector kernel, bits 16-23: the same for the L^T product of
 * M = L L^T --, 4 the colour sweeps of a triangular solve: out[12] launches that add to <r,z> (the levels of the upper solve, first
 * to last), out[13] workgroups of each, out[14] two bits per launch, first launch lowest (how a workgroup walks the level's 256-row
 * blocks: 0 its slab by virtual block, 1 blocks b, b + G, ..., 2 the same by virtual block), out[15] = 1 when the first of them is the
 * lower solve's last launch --, 9 a tree the checker does not restate: more than 16 sweeps). */
int dpcg_get_reduction_geometry(dpcg_handle_t h, int32_t out[16]);
/* The whole-chip solve (dpcg_chip.hip: 65 537 .. 1 048 576 rows, M = I / Jacobi, cg.py:58-90 in ONE launch of 256 workgroups -- rows of
 * <= 7 entries (9 up to 524 288 rows) within 32 767 columns of the diagonal: matrix and vectors stay in registers and LDS for the whole
 * solve; otherwise, rows of <= 24 entries: the vectors stay, the matrix is streamed every update; the same rows per thread and the same
 * reduction trees either way).  out[0] = 1 when the
 * system with its CURRENT preconditioner is eligible (2: and a plain dpcg_solve takes that form), out[1] = workgroups (256),
 * out[2] = threads of each (512), out[3] = rows per workgroup (ceil(n / 256): workgroup v owns rows v * out[3] .., thread t of it
 * rows v * out[3] + t + 512 k -- what a checker needs to add the dot products in the kernel's order), out[4] = longest row,
 * out[5] = largest |col - row| (-1: not measured, systems beyond 1 048 576 rows), out[6]: bit 0 = the last traced chip solve found
 * every group of 32 workgroups on one XCD (and kept plainly stored copies in that XCD's L2), bits 8-15 = lanes that share a row (2: M = L L^T
 * multiplied with 16-entry factor rows; row v * out[3] + t / 2 then speaks through the even lane t of its pair in the dot products), out[7] = with DPCG_CHIP_EVENTS=1 in the
 * environment, the duration of the last chip kernel in nanoseconds, between HIP events on the stream it ran on.  trace_us (may be NULL): with DPCG_CHIP_TRACE=1 in
 * the environment, microseconds per update that workgroup 0 spent in the phases of the last chip solve -- [0] q = A p (the SpMV
 * phase), [1] sum <p,Ap> incl. its barrier, [2] vector updates + publishing, [3] sum <r,z>, <r,r> incl. its barrier, [4] the whole
 * loop, [5] / [6] of [1] / [3]: waiting for the other workgroups' slots, [7] = the number of updates.  No reference counterpart
 * (the reference's loop is host Python, cg.py:70-87).  A DPCG_SINGLE_REDUCTION solve has no phase timing: it zeroes trace_us and
 * bit 0 of out[6], and out[7] unless DPCG_CHIP_EVENTS=1 measured that kernel.  out[8] of out[9]: where the handle's LAST solve was a resident
 * standard chip solve, the (wave, slot-row) pairs of it that took the operands their wave holds (the own rows' p and those of the rows beside
 * them) from its registers instead of gathering them, of the pairs that have a row at all (DPCG_CHIP_SHARED=0 in the environment: 0 of them);
 * 0 of 0 after any other solve. */
int dpcg_get_chip_info(dpcg_handle_t h, int32_t out[10], double trace_us[8]);
/* The recurrence the handle's last dpcg_solve / dpcg_solve_batch member ran: 0 = the standard one (cg.py:70-87), 1 = the
 * single-reduction one (DPCG_SINGLE_REDUCTION).  0 before the first solve.  No reference counterpart. */
int dpcg_get_last_recurrence(dpcg_handle_t h, int *recurrence);
/* Test hook: enqueue on `stream` a kernel of `workgroups` workgroups that each take a whole CU (all of its LDS) and spin for
 * `milliseconds` -- what a long-running kernel of another stream or process does to the co-residency the one-launch solves (team,
 * chip) rely on.  They bound every wait (20 ms) and fall back to the multi-launch path; the tests hold them to that with this call.
 * No reference counterpart. */
int dpcg_debug_occupy(int workgroups, double milliseconds, dpcg_stream_t stream);
/* Measurement hook (bench.py `roofline.frac_of_measured_ceiling`): the rate at which the chip serves what the whole-chip solve kernel
 * (dpcg_chip.hip) gathers -- 16-byte granules stored plainly by the workgroups of the owner's XCD, read with agent-scope loads, 64
 * consecutive granules per wave instruction -- with nothing else going on: 256 workgroups x 512 threads, `granules_per_group` granules per
 * XCD (a multiple of 32, >= 16 384), `reps` passes of 8 x 7 gathers per thread at `offsets` (in granules, relative to the thread's rows,
 * wrapped inside the XCD's part), `depth` (2 | 4) rows' gathers in flight per lane; `written_through` = 1: the table written through
 * instead of plainly (the lines still stay in the writer's L2); 2: written through AND gathered by the neighbouring XCD (every gather
 * then leaves the L2 for the memory side: the path of the granules another XCD owns).  Out: GB/s of gathered bytes, us per pass, whether every group sat on one XCD.
 * DPCG_ERR_STATE when the workgroups could not be co-resident.  No reference counterpart. */
int dpcg_debug_l2_gather(int granules_per_group, int reps, const int32_t offsets[7], int depth, int written_through, dpcg_stream_t stream,
                         double *gbs, double *us_per_pass, int *groups_local);
/* Copy the current factor L out (host arrays sized from dpcg_get_info's precond_nnz). */
int dpcg_get_factor(dpcg_handle_t h, int32_t *rowptr, int32_t *col, double *val);

/* ---- standalone operators (roofline benches, unit parity, duck-typed `@`) -------------------- */
int dpcg_spmv(dpcg_handle_t h, const double *x, double *y, dpcg_stream_t stream);          /* cg.py:60,75 */
int dpcg_spmv_f32(dpcg_handle_t h, const float *x, float *y, dpcg_stream_t stream);        /* config C5   */
int dpcg_precond_apply(dpcg_handle_t h, const double *r, double *z, dpcg_stream_t stream); /* cg.py:61,81 */
int dpcg_sptrsv(dpcg_handle_t h, int upper, const double *rhs, double *out, dpcg_stream_t stream);
/* *out_host = <a,b> (torch.inner, cg.py:17,76,78,82); deterministic two-stage reduction. */
int dpcg_dot(int64_t n, const double *a, const double *b, double *out_host, dpcg_stream_t stream);
/* The SpMV fused with <p,Ap> exactly as launched inside the PCG iteration (for kernel timing). */
/* (times the kernel a default solve launches: with two-kernel updates that is the SpMV fused with the vector update) */
int dpcg_spmv_dot_bench(dpcg_handle_t h, const double *x, double *y, int repeats, float *ms_per_launch,
                        dpcg_stream_t stream);

/* The HBM streaming ceiling of this box with the library's own access shape (SURVEY.md 8-d2 asks for a measured ceiling
 * beside the 8 TB/s spec; nothing in the reference corresponds -- its loop runs on torch CPU/CUDA ops, cg.py:75-86): per 16
 * bytes written, n_read x 16 contiguous bytes are read (n_read = 1 copy, 2 triad, 4, or 11 = the read:write ratio of a
 * 7-point CSR SpMV); write = 0: read-only, n_read x out_bytes are only reduced.  nontemporal: bit 0 = non-temporal loads and
 * stores; bit 1 = the streams are WALKED TOGETHER by the whole grid (workgroup b takes pieces b, b + G, ...) instead of one
 * contiguous slab per workgroup -- a copy then is one 16-byte element per thread, the "float4 copy" MI355X_MICROARCH.md quotes
 * 6.29 TB/s for (measured here: 6.3; slabs 5.3).  `repeats` launches between HIP events on `stream`; *bytes_per_launch = reads + writes of one launch. */
int dpcg_stream_bench(int n_read, int write, int nontemporal, int64_t out_bytes, int repeats, float *ms_per_launch,
                      int64_t *bytes_per_launch, dpcg_stream_t stream);

/* ---- spectrum of M A: test.py:111-113 (kappa = cond(M @ A)) at any size -------------------------------------------
 * The reference forms M A densely and takes cond() of it; this runs a Lanczos process in the M inner product on the device
 * (M A is similar to the symmetric M^{1/2} A M^{1/2}), with full reorthogonalisation (CGS2) against a basis resident in HBM,
 * for whatever symmetric positive definite M the handle applies (Jacobi, CSR, L L^T multiplied or solved, a callback).  The
 * start vector is a counter-based hash of (seed, the caller's row index): results do not depend on the handle's numbering and
 * two calls give the same bits.  Out: *steps, the extreme Ritz values theta_min / theta_max (eigenvalues of M A; kappa =
 * theta_max / theta_min -- lambda_max / lambda_min, which equals the reference's singular-value ratio only when M = c I),
 * their error bounds err = beta_{k+1} |s_k| (s_k: last component of the Ritz vector in T_k); alpha, beta (host, >= min(max_steps,
 * n) doubles each, or NULL): the diagonal and the off-diagonals of T_k, beta[k-1] = beta_{k+1}.  At most min(max_steps, n)
 * steps; stops when both bounds are <= rtol |theta|, when beta reaches 0 or after n steps (exact: DPCG_OK), else DPCG_MAX_ITER.
 * DPCG_BREAKDOWN: <w, M w> <= 0 beyond rounding (M is not positive definite) or a non-finite value; no number is returned.
 * DPCG_ERR_NOMEM: the basis, 2 x (max_steps + 1) x n doubles, does not fit.  Synchronises `stream` every 16 steps and on return;
 * leaves the handle's solve state alone (its own buffers, from the block cache). */
int dpcg_spectrum(dpcg_handle_t h, int max_steps, double rtol, uint64_t seed, dpcg_stream_t stream, int *steps,
                  double *theta_min, double *theta_max, double *err_min, double *err_max,
                  double *alpha, double *beta);
/* Host only: eigenvalues theta[0..k) (ascending) of the symmetric tridiagonal with diagonal alpha[0..k) and off-diagonal
 * beta[0..k-1) (beta may be NULL when k = 1), and bottom[i] = the last component of theta[i]'s unit eigenvector (sign
 * arbitrary).  Implicit QL with Wilkinson shifts. */
int dpcg_tridiag_ritz(int k, const double *alpha, const double *beta, double *theta, double *bottom);
/* Host only: the nvec lowest eigenpairs of the same tridiagonal (1 <= nvec <= k), theta[0..nvec) ascending and S column-major k x nvec,
 * S[i * k + r] = component r of theta[i]'s unit eigenvector (sign arbitrary).  The same QL iteration with the rotations accumulated on
 * the whole eigenvector matrix: O(k^2) per sweep, the eigenvalues bit-equal to dpcg_tridiag_ritz's. */
int dpcg_tridiag_eigvecs(int k, const double *alpha, const double *beta, int nvec, double *theta, double *S);
/* The k lowest Ritz vectors of M A (1 <= k <= 8), harvested from the same Lanczos process as dpcg_spectrum -- the same start vector,
 * the same step kernels, the basis Z = M R resident in HBM -- for use as deflation vectors (dpcg_set_deflation, below).  Stops when the
 * k lowest Ritz pairs have err_i <= rtol theta_i, when beta reaches 0 or after n steps (DPCG_OK), or after max_steps (DPCG_MAX_ITER: the
 * vectors are returned all the same).  theta[k], err[k] (host): the Ritz values, ascending, and their bounds beta_{m+1} |s_m|.  W_dev:
 * device fp64, column-major n x k in the CALLER's numbering: y_i = Z s_i, s_i the unit eigenvector of T_m (dpcg_tridiag_eigvecs), one
 * pass over the basis columns, every sum in column order.  The y_i are M-orthonormal approximations of eigenvectors of M A, not yet
 * A-orthonormal.  DPCG_ERR_INVALID when the Krylov space of the start vector has fewer than k dimensions; otherwise as dpcg_spectrum. */
int dpcg_spectrum_vectors(dpcg_handle_t h, int k, int max_steps, double rtol, uint64_t seed, dpcg_stream_t stream, int *steps,
                          double *theta, double *err, double *W_dev);

/* ---- projected initial guess for a SEQUENCE of systems on one handle ------------------------------------------------
 * The reference starts every solve from zeros (cg.py:58).  In a time-stepping run ("same mesh, next time step") consecutive
 * solutions lie close to the span of the last few; P. F. Fischer's projection (CMAME 163, 1998) starts the next solve from the
 * A-norm-best approximation in that span.  The object keeps, per system, a basis X~ = [x~_0 .. x~_{l-1}], l <= depth, with
 * x~_i^T A x~_j = delta_ij, and W = A X~, both on the device and in the CALLER's numbering (dpcg_reorder does not touch them).
 *   project(b): c = X~^T b, x0 = X~ c (l = 0: zeros).  x0: device fp64[n], out; the object keeps a copy for the next update.
 *   update(x):  d = x - x0, w = A d (the handle's SpMV), classical Gram-Schmidt twice in the A inner product (g = X~^T w,
 *     d -= X~ g, w -= W g), s = <d, w>.  The direction is dependent -- skipped, the size stays -- when s <= tol_dep^2 <x, A x>
 *     or s is not finite; otherwise d / sqrt(s) and w / sqrt(s) are appended.  A full basis (l == depth) restarts instead, as
 *     Fischer does: it becomes the single vector x / ||x||_A (one SpMV).  The x0 of the last project is used only while the
 *     basis it was formed from stands (no restart, re-orthonormalisation or reset in between); otherwise d = x.
 *   new matrix values: dpcg_update_values moves the handle's values epoch; the next project (or update) sees that its own copy
 *     is behind and first makes the basis consistent: W = A X~ by l SpMVs, then twice (CholQR2) the Gram matrix G = X~^T W on
 *     the device, G = R^T R on the host -- direction j and all later ones are dropped at the first pivot <= tol_dep^2 G_jj --
 *     and X~ <- X~ R^-1, W <- W R^-1 in place on the device.
 * depth 1 .. 32, tol_dep > 0 (1e-7 is a good default); otherwise DPCG_ERR_INVALID.  Memory: 2 x depth x ld doubles from the block
 * cache, ld = n rounded up to a multiple of 1024 (DPCG_ERR_NOMEM when they do not fit).  Every sum has one fixed order (no float
 * atomics): the same sequence gives the same bits.  project and update read scalars back: each synchronises `stream` once.
 * A non-finite value in b or x is DPCG_ERR_INVALID and leaves the basis (and the kept x0) as it was.  One thread and one stream
 * at a time, as for the handle.  After dpcg_destroy of the system every call but dpcg_guess_destroy returns DPCG_ERR_STATE.
 * dpcg_guess_reset empties the basis and the counters.  dpcg_guess_info: out = {depth, size, restarts, appended, skipped as
 * dependent, dropped at a re-orthonormalisation, re-orthonormalisations (one per change of the matrix the object has seen,
 * whatever the size), the values epoch the basis is consistent with}.  dpcg_guess_get_basis (for tests): the `size` columns of
 * X~ and of W, column-major with n rows each, into host arrays (either may be NULL); waits for the device. */
typedef struct dpcg_guess *dpcg_guess_t;
int dpcg_guess_create(dpcg_handle_t h, int depth, double tol_dep, dpcg_guess_t *out);
int dpcg_guess_project(dpcg_guess_t g, const double *b, double *x0, dpcg_stream_t stream);
int dpcg_guess_update(dpcg_guess_t g, const double *x, dpcg_stream_t stream);
int dpcg_guess_reset(dpcg_guess_t g);
int dpcg_guess_info(dpcg_guess_t g, int32_t out[8]);
int dpcg_guess_get_basis(dpcg_guess_t g, double *X_host, double *W_host);
int dpcg_guess_destroy(dpcg_guess_t g);

/* ---- the solve: cg.py:50-90 (PCG) and cg.py:20-47 (CG = PCG with M = I, test on r) ----------- */
/*
 * b, x0 (may be NULL = zeros, cg.py:58), x (out, may be NULL): device fp64[n].  x is written in stream order: valid for
 * work enqueued on `stream` after the call, and for the host once `stream` is synchronised (the scalar outputs and the
 * host-side histories are complete on return).
 * Stop when res_k = <r_k,r_k>/<b,b> < rtol_sq or <r_k,r_k> < atol_sq (cg.py:15-17,71: SQUARED
 * ratio; atol_sq = 0 for the reference, 1e-12 for generate_data.py:107), k = 0 tested on
 * <z_0,z_0>/<b,b> unless DPCG_INIT_CHECK_R (cg.py:66).  At most max_iter updates (cg.py:70).
 * iters = completed updates = len(errors)-1 (cg.py:90).  seconds = host wall time around the
 * iteration loop, device-synchronised (cg.py:69,88).  res_history: host fp64[max_iter+1] or NULL,
 * entry k is what the reference appends to `errors` (cg.py:67,88).
 * x_true / err_history (both NULL for PCG): when given, err_history[k] = (x_k-x_true)^T A (x_k-x_true)
 * (cg.py:27-29,43-45), one extra SpMV per iteration as in the reference.
 * Returns DPCG_OK / DPCG_MAX_ITER / DPCG_BREAKDOWN or a negative error.
 */
int dpcg_solve(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq, double atol_sq,
               int max_iter, int flags, dpcg_stream_t stream, int *iters, double *final_res, double *seconds,
               double *res_history, const double *x_true, double *err_history);

/* ---- singular systems: a null space attached to the handle, projected inside PCG -------------------------------------
 * A closed domain (all-Neumann boundaries, or several closed regions in one mesh) gives a symmetric positive SEMI-definite
 * matrix whose kernel is the constants (one constant per region).  Not in the reference, whose systems are all definite.
 * With Z (n x k, orthonormal columns, 1 <= k <= 4) attached and P = I - Z Z^T, dpcg_solve runs
 *     b' = P b;  r = b' - A x0 (x0 given: r = P r once);  bb = <b',b'>;  zt = M r;  s = Z^T zt;  t = Z^T r;
 *     rho = <r,zt> - t^T s;  p = zt - Z s;   first test: <p,p> = <zt,zt> - s^T s, or <r,r> with DPCG_INIT_CHECK_R
 *     each update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q
 *                   zt = M r                      (NOT projected in memory)
 *                   s = Z^T zt;  t = Z^T r        (k numbers each)
 *                   rho' = <r,zt> - t^T s         (= <r, P zt>)
 *                   p = (zt - Z s) + (rho'/rho) p (the projection lives only in this update)
 *     end:          x = x - Z (Z^T x)             (the minimum-norm solution; also after max_iter updates and after a breakdown)
 * The history, the stopping test, the first test, the cap and the NaN breakdown mean what they mean above, with b' for b.
 * An update is the SpMV with its partials of <p,q>, one pass over q, r (dinv) that leaves per-workgroup partials of <r,zt>, <r,r>,
 * Z^T zt and Z^T r (2 + 2k sums, each summed in one fixed order: no float atomics), and one pass over r (dinv), p, x -- for M = I
 * and Jacobi the launches and reduction rounds of a definite solve.  Any other M: the r update, the handle's apply, one dot kernel.
 *
 * dpcg_set_nullspace: k = 0 clears.  Z == NULL with k == 1: the constant vector 1/sqrt(n), never read from memory (the vector
 * passes then move the bytes of a definite solve; a general Z adds 8k bytes per row to each).  Otherwise Z is column-major n x k
 * (memspace as for dpcg_create) in the CALLER's numbering, any linearly independent columns: the library orthonormalises them on
 * the host (fp64 modified Gram-Schmidt, twice) and permutes them to the handle's numbering when the handle is reordered
 * (dpcg_reorder on a handle that has a null space is DPCG_ERR_STATE: reorder first).  check_tol > 0: every column must satisfy
 * max_i |(A z_j)_i| <= check_tol ||A||_inf ||z_j||_inf; check_tol <= 0: no check.  DPCG_ERR_INVALID (text in dpcg_last_error) for
 * k < 0 or k > 4, Z == NULL with k > 1, a non-finite entry, a rank-deficient Z (a column's norm after orthogonalisation below
 * 1e-12 of its norm before) and a failed check; the handle then keeps what it had.  dpcg_update_values keeps the null space and
 * repeats the check when one was asked for (its failure is that call's DPCG_ERR_INVALID; the null space is then dropped).
 * dpcg_get_nullspace: *k (0: none) and, Z_host != NULL, the orthonormal basis column-major n x k in the caller's numbering.
 *
 * A handle with a null space takes this driver whatever its size (no one-launch form).  Refused with DPCG_ERR_INVALID and a reason:
 * DPCG_SINGLE_REDUCTION, DPCG_SPMV_F32, DPCG_TEAM; x_true; dpcg_solve_batch with such a handle; DPCG_PRECOND_AMG (its exact coarse
 * solve inverts a singular matrix); DPCG_PRECOND_CALLBACK (the driver enqueues updates ahead of the test and a callback cannot be
 * skipped once it has passed).  A handle without a null space takes exactly the paths it took. */
int dpcg_set_nullspace(dpcg_handle_t h, int k, const double *Z, int memspace, double check_tol, dpcg_stream_t stream);
int dpcg_get_nullspace(dpcg_handle_t h, int *k, double *Z_host);

/* ---- deflated PCG: a few vectors attached to the handle and projected out of the search directions --------------------
 * A handful of smallest eigenvalues of M A sets the update count on Poisson-type systems, and no preconditioner here removes them.
 * Deflation does (Saad, Yeung, Erhel, Guyomarc'h, SISC 21, 2000; with piecewise-constant vectors: Nicolaides' subdomain deflation).
 * Not in the reference.  With W (n x k, 1 <= k <= 8, W^T A W = I -- the library makes it so) and AW = A W attached, dpcg_solve runs
 *     start:   r = b - A x0 (x0 NULL: r = b);  c = W^T r;  x = x0 + W c;  r = r - AW c        (no second SpMV)
 *              bb = <b,b> of the caller's b;  z = M r;  mu = AW^T z;  p = z - W mu;  rho = <r,z>
 *              first test: <z,z>/bb, or <r,r>/bb with DPCG_INIT_CHECK_R, on the r AFTER the start correction
 *     update:  q = A p;  alpha = rho / <p,q>;  x += alpha p;  r -= alpha q;  z = M r
 *              mu = AW^T z  (k sums);  rho' = <r,z>;  p = (z - W mu) + (rho'/rho) p
 * The history, the stopping test, the cap, the NaN breakdown and the status words mean what they mean for dpcg_solve above.
 * An update is the SpMV with its partials of <p,q>, one pass over q, r (dinv), AW that leaves per-workgroup partials of <r,r>, <r,z> and
 * AW^T z (2 + k sums, each summed in one fixed order: no float atomics), and one pass over r (dinv), p, x, W -- for M = I and Jacobi the
 * launches and reduction rounds of a plain solve, 8 k more bytes per row in each of the two passes.  Any other M: the r update, the
 * handle's apply, one dot kernel.
 *
 * dpcg_set_deflation: k = 0 clears.  W is column-major n x k (memspace as for dpcg_create) in the CALLER's numbering, any columns that
 * are linearly independent: the library checks that every entry is finite, permutes W to the handle's numbering, forms AW by k calls of
 * the handle's SpMV and A-orthonormalises by CholQR2 as the projected guess does after new values (G = W^T AW on the device with
 * fixed-order sums, Cholesky on the host, W <- W R^-1 and AW <- AW R^-1 in place, twice).  Unlike the guess, a dependent column -- a
 * pivot <= tol^2 G_jj, tol = 1e-7 -- is refused, not dropped: DPCG_ERR_INVALID, the text names the column.  k < 0, k > 8 and a
 * non-finite entry are DPCG_ERR_INVALID too; after any refusal the handle keeps what it had.  Columns are stored ld rows apart (ld = n
 * rounded up to a multiple of 1024: every column 16-byte aligned), the padding zero.  dpcg_update_values keeps the span: it recomputes AW
 * and the A-orthonormalisation before it returns (a failure is that call's DPCG_ERR_INVALID; the deflation is then dropped).
 * dpcg_reorder on a handle that carries a deflation is DPCG_ERR_STATE: reorder first.  dpcg_set_preconditioner keeps the vectors.
 * dpcg_get_deflation: *k (0: none) and, where not NULL, the A-orthonormal W and AW as the device holds them, column-major n x k in the
 * caller's numbering (host); waits for the device.
 *
 * A handle with a deflation takes this driver whatever its size (no one-launch form deflates).  Refused with DPCG_ERR_INVALID and a
 * reason: DPCG_SINGLE_REDUCTION, DPCG_SPMV_F32, DPCG_TEAM; x_true; dpcg_solve_batch with such a handle; DPCG_PRECOND_CALLBACK; a handle
 * that also has a null space (refused at whichever attach comes second).  DPCG_PRECOND_AMG is accepted.  A handle without a deflation
 * takes exactly the paths it took. */
int dpcg_set_deflation(dpcg_handle_t h, int k, const double *W, int memspace, dpcg_stream_t stream);
int dpcg_get_deflation(dpcg_handle_t h, int *k, double *W_host, double *AW_host);

/* ---- mixed-precision PCG: fp32 inner iterations inside an fp64 refinement loop ------------------------------------------
 * PCG whose vectors and matrix values are all STORED in fp32, wrapped in an fp64 loop that recomputes the true residual and
 * corrects x (iterative refinement).  Not in the reference.  Storage is fp32 and arithmetic is fp64 (the convention of the fp32 AMG
 * cycle): every product and sum is formed in fp64, a value is rounded to fp32 exactly where it is stored to an fp32 vector.
 *     A32 = fl32(A values), dinv32 = fl32(1/a_ii) (Jacobi)      made by the first call, kept until the values, the preconditioner or
 *                                                                the numbering change
 *     bb = <b,b> (fp64);  x = x0 or 0 (fp64);  total = 0
 *     outer s = 0, 1, ...:
 *         r = b - A x                                  fp64, the handle's fp64 SpMV (x0 == NULL, s = 0: r = b)
 *         rr = <r,r>;  outer_history[s] = rr / bb
 *         stop OK        if rr/bb < rtol_sq or rr < atol_sq
 *         stop MAX_ITER  if total == max_iter or s == max_outer
 *         stop BREAKDOWN if rr is not finite or rr / bb is not a number
 *         stop MAX_ITER  ("stagnated" in dpcg_last_error) if s >= 1 and rr >= 0.25 * rr_prev
 *         sigma = sqrt(rr);  r32 = fl32(r / sigma)     (scaled: the inner problem never drifts into fp32 denormals)
 *         target = max(inner_rtol_sq, 0.25 * rtol_sq * bb / rr)     (the last outer step does not over-solve)
 *         inner PCG on A32 d = r32 from d = 0 with M = I or diag(dinv32): the recurrence of dpcg_solve with DPCG_INIT_CHECK_R
 *             z = fl32(dinv32 r);  p = z;  rho = <r,z>;  first test on <r,r>
 *             update:  q = fl32(A32 p);  alpha = rho / <p,q>;  d = fl32(d + alpha p);  r = fl32(r - alpha q);  z = fl32(dinv32 r);
 *                      rho' = <r,z>;  p = fl32(z + (rho'/rho) p);  test <r,r> / <r32,r32> < target
 *             at most max_iter - total updates;  d, r, z, p, q are fp32 vectors (z is never stored: both readers form the same
 *             rounded product);  alpha, beta and all dots are fp64, the dots over the STORED (rounded) vectors
 *         total += inner updates;  x += sigma * d      fp64
 * iters = total, the inner updates summed over all outer steps.  outer = the number of outer residual evaluations minus one (= the
 * number of inner solves).  final_res = the last rr / bb: a TRUE residual, not a recurrence value, and equal to the last entry
 * written to outer_history.  outer_history: host fp64[max_outer + 1] or NULL, entries 0 .. outer.  res_history: host
 * fp64[max_iter + 1] or NULL, iters + 1 entries: entry 0 is outer_history[0], and entry t >= 1 is the inner recurrence's <r,r>
 * after update t rescaled to the outer problem, <r,r> * rr / bb with the rr of the outer step the update belongs to -- the
 * histories of successive outer steps concatenated, one entry per update (an inner solve's own first entry, which restates the
 * outer value it starts from, is not repeated).  seconds = host wall time around the whole outer loop, device-synchronised.
 * <b,b> == 0 behaves as in dpcg_solve: from x0 == NULL or an x0 with A x0 == 0, rr / bb is 0/0, not a number, so the first test is
 * OK only through atol_sq > 0, DPCG_MAX_ITER with max_iter == 0 (the tests run in the order above) and DPCG_BREAKDOWN otherwise, with
 * x = x0 or 0 and no update done.  (From any other x0 it is rr / 0 = +inf: never OK through rtol_sq, and no breakdown.)  A b that
 * holds a NaN or an infinity stops the same way at the first test.  inner_rtol_sq > 1 makes every inner solve one of zero updates
 * (its first test, 1 < target, passes): x stays as it is and the next outer test ends the call "stagnated".
 * An inner solve that breaks down -- <p,q> is 0 or not finite, as when every value of A rounds to 0 in fp32 (finite, so not
 * refused) -- ends at that update, which is counted and whose history entry is NaN; its d, not finite, is added to x as it is, and
 * the next outer residual, not finite either, stops the call with DPCG_BREAKDOWN.
 * An inner update is three launches as in the plain solve: a CSR row SpMV over fp32 values and fp32 p with its partials of <p,q>,
 * one pass over q, r (dinv32) that leaves per-workgroup partials of <r,r> and <r,z>, one pass over r (dinv32), p, d -- 4 bytes a
 * vector entry where the fp64 launches move 8, 8 bytes a non-zero where they move 12.  Each sum is formed in one fixed order: no
 * float atomics.  An outer step adds the fp64 SpMV, one pass that forms r and its partials, one that scales it to fp32 and starts
 * the inner solve, and one that adds sigma d to x; the host reads rr once per outer step.
 * flags: 0 or DPCG_NO_GRAPH (accepted; this driver replays no graph).  Refused with DPCG_ERR_INVALID and a reason in
 * dpcg_last_error, the handle unchanged: a preconditioner other than none or Jacobi; a handle with a null space or a deflation; any
 * other flag; inner_rtol_sq <= 0, max_outer < 1, max_iter < 0; a matrix value or reciprocal diagonal that is not finite after
 * rounding to fp32 (the text names the first such entry, in the handle's numbering).  A reordered handle works as for dpcg_solve:
 * b, x0 and x are gathered and scattered, the inner solve runs in the handle's numbering.  dpcg_solve and every other entry point
 * keep their paths and bits.  Returns DPCG_OK / DPCG_MAX_ITER / DPCG_BREAKDOWN or a negative error. */
int dpcg_solve_refined(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq, double atol_sq,
                       int max_iter, double inner_rtol_sq, int max_outer, int flags, dpcg_stream_t stream,
                       int *iters, int *outer, double *final_res, double *seconds, double *res_history, double *outer_history);

/* ---- BiCGStab: systems whose VALUES are not symmetric, and preconditioners that are not ------------------------------------
 * Every other solve form here is a conjugate-gradient recurrence and needs a symmetric positive definite A and a symmetric M.  This
 * one is right-preconditioned BiCGStab (van der Vorst, SIAM J. Sci. Stat. Comput. 13, 1992), what OpenFOAM pairs PCG with (PBiCGStab)
 * for its momentum and phase-fraction matrices: a structurally symmetric pattern with non-symmetric values.  Not in the reference.
 * Right-preconditioned: the residual it recurs is the residual of the ORIGINAL system.
 *     r0 = b - A x0;  rhat = r0;  bb = <b,b>;  rho = alpha = omega = 1;  v = p = 0;  history[0] = <r0,r0>/bb, tested (always on r:
 *                                                                                     there is no z0 quirk here)
 *     update k:  rho' = <rhat,r>;  beta = (rho'/rho)(alpha/omega);  rho = rho'
 *                p = r + beta (p - omega v);  ph = M p;  v = A ph;  alpha = rho / <rhat,v>
 *                s = r - alpha v;  ss = <s,s>
 *                if ss meets the test:  x += alpha ph;  history[k+1] = ss/bb;  count = k+1;  stop (DPCG_OK)
 *                sh = M s;  t = A sh;  omega = <t,s>/<t,t>
 *                x += alpha ph + omega sh  (as (x + alpha ph) + omega sh);  r = s - omega t;  history[k+1] = <r,r>/bb;  test
 * The pointer rules, the stream semantics, `seconds`, the squared-ratio test (res < rtol_sq or <r,r> < atol_sq) and the meaning of
 * iters / final_res / res_history are dpcg_solve's.  DPCG_BREAKDOWN: rho', <rhat,v> or <t,t> is exactly zero, or one of the sums is not
 * finite (a history entry that is not a number included, as for <b,b> = 0); x is then the last iterate that was completed, iters its
 * index, and the history ends there.  DPCG_MAX_ITER after max_iter updates; max_iter = 0 tests r0 only.  (omega = 0 is not examined: the
 * next update's sums are then not finite and end the solve.)
 * An update is the launches P | v = A ph | S | t = A sh | <t,t> | X: three fused vector passes (dpcg_bicgstab.hip) around the handle's own
 * SpMV, whose epilogue leaves the partials of <rhat,v> and of <s,t>; M = I and Jacobi are fused into the passes, any other M runs as the
 * pass, the handle's apply (dpcg_precond_apply's internals), the SpMV.  The scalars live on the device and every decision -- the test, the
 * half-step exit, a breakdown -- is taken there; the host keeps updates enqueued ahead of a progress word, at most max_iter of them.
 * Every dot product is per-workgroup partials summed in one fixed order (no float atomics): two runs of the same call give the same bits.
 * A: any CSR dpcg_create accepts; a reordered handle works as in dpcg_solve (b, x0, x keep the caller's numbering).
 * M: DPCG_PRECOND_NONE, JACOBI, CSR, LLT_MULTIPLY, LLT_SOLVE, LU_MULTIPLY, LU_SOLVE, BLOCK_LLT_SOLVE and AMG; no symmetry is asked of it.
 * flags: 0 or DPCG_NO_GRAPH (accepted; this driver replays no graph).  Refused with DPCG_ERR_INVALID and a reason in dpcg_last_error,
 * the handle unchanged: DPCG_PRECOND_CALLBACK (the driver enqueues updates ahead of the test and a callback cannot be skipped once it has
 * passed); a handle with a null space or a deflation; any other flag; a tolerance that is not finite; max_iter < 0.  dpcg_solve and
 * every other entry point keep their paths and bits.  Returns DPCG_OK / DPCG_MAX_ITER / DPCG_BREAKDOWN or a negative error. */
int dpcg_solve_bicgstab(dpcg_handle_t h, const double *b, const double *x0, double *x, double rtol_sq, double atol_sq,
                        int max_iter, int flags, dpcg_stream_t stream, int *iters, double *final_res, double *seconds,
                        double *res_history);

/* `count` independent systems (train.py:90-108 / test.py:121-149 loop over samples): handles[i],
 * b[i], x0[i], x[i] as above; outputs are arrays of length count.  Systems are interleaved on
 * `n_streams` internal streams (1..8).  Returns the worst status. */
int dpcg_solve_batch(int count, dpcg_handle_t *handles, const double *const *b, const double *const *x0,
                     double *const *x, double rtol_sq, double atol_sq, int max_iter, int flags, int n_streams,
                     int *iters, double *final_res, double *seconds, int *status);

/* ---- synthetic pressure-Poisson systems generated on the device -------------- */
/* dim = 2: 5-point, n*n rows; dim = 3: 7-point, n^3 rows.  Sizes via dpcg_poisson_sizes. */
int dpcg_poisson_sizes(int dim, int64_t n, int64_t *rows, int64_t *nnz);
int dpcg_gen_poisson(int dim, int64_t n, int32_t *rowptr, int32_t *col, void *val, int val_dtype,
                     dpcg_stream_t stream);

/* ---- sparse_matvec_mul (utils.py:15-43): batched COO SpMV / SpMV^T, fp32 ---------------------- */
/* indices: int32[nnz*3] rows of (batch,row,col); features fp32[nnz]; vectors/out fp32[batch*dof].
 *
 * Two guards hold for the four dpcg_batched_coo_* entry points below:
 *   range:  a triple with batch_k outside [0, batch) or row_k / col_k outside [0, dof) is not an error.  spmv and spmm SKIP it
 *           (it adds nothing to `out`); edge and sddmm, which own out[k], write out[k] = 0.0f.  No operand is read for it.
 *   zero:   spmm alone skips a triple whose features[k] == 0.0f (+0 or -0: the masked upper triangle of the network output),
 *           so a non-finite panel entry under an explicit zero stays out of the result.  spmv has no such test: there
 *           0 * inf and 0 * NaN are NaN, as IEEE 754 has them.  edge and sddmm read no feature.
 * Duplicate triples are legal and add up (fp32 atomics: the order of the additions, and so the last bits, vary from run to run). */
int dpcg_batched_coo_spmv(int64_t nnz, const int32_t *indices, const float *features, int batch, int64_t dof,
                          const float *vectors, float *out, int transpose, dpcg_stream_t stream);

/* Gradient of sparse_matvec_mul w.r.t. the matrix entries (training through frobenius_loss, metrics.py:28-29):
 * out[k] = a[batch_k, row_k] * c[batch_k, col_k] with (row,col) as in dpcg_batched_coo_spmv for `transpose`: ONE fp32
 * product, the same bits on every run.  A triple out of range gives out[k] = 0.0f (the range guard above). */
int dpcg_batched_coo_edge(int64_t nnz, const int32_t *indices, int batch, int64_t dof, const float *a, const float *c,
                          float *out, int transpose, dpcg_stream_t stream);

/* The same two operators on PANELS of `ncols` right-hand sides (fp32[batch*dof*ncols], row-major [b][row][c]): the
 * building blocks of `inverse_loss` (metrics.py:34-55, the loss train.py:59 minimises) WITHOUT the reference's dense
 * N x N products: || L L^T A - I ||_F is accumulated over panels of columns J as L (L^T A[:, J]) - I[:, J].
 * spmm: out[b, row_k, :] += features[k] * panel[b, col_k, :]; sddmm: out[k] = <g[b, row_k, :], panel[b, col_k, :]> (the
 * gradient of spmm with respect to features[k]).  (row, col) swap under `transpose` as in dpcg_batched_coo_spmv.
 * Guards as stated there: spmm skips a triple out of range AND a triple with features[k] == 0.0f; sddmm writes out[k] = 0.0f
 * for a triple out of range and has no zero test (its result for a zero feature is the full dot product). */
int dpcg_batched_coo_spmm(int64_t nnz, const int32_t *indices, const float *features, int batch, int64_t dof, int ncols,
                          const float *panel, float *out, int transpose, dpcg_stream_t stream);
int dpcg_batched_coo_sddmm(int64_t nnz, const int32_t *indices, int batch, int64_t dof, int ncols, const float *g,
                           const float *panel, float *out, int transpose, dpcg_stream_t stream);

/* ---- coordinate triplets -> CSR on the device (the reference's file formats are COO: scipy npz,
 * generate_data.py:109; OpenFOAM `i,j,value` dump, pEqn.H:98-108; StAn npz, data_set.py:186-188) ------------- */
/* rows/cols int32[nnz], vals fp64[nnz]: device.  Stable sort by (row,col), duplicates summed in storage order.
 * rowptr int32[n+1], col_out int32[nnz], val_out fp64[nnz]: device, capacity nnz; *nnz_out = unique entries. */
int dpcg_coo_to_csr(int64_t n, int64_t nnz, const int32_t *rows, const int32_t *cols, const double *vals,
                    int32_t *rowptr, int32_t *col_out, double *val_out, int64_t *nnz_out, dpcg_stream_t stream);

/* ---- the CNN that emits L: PreconditionerNet's sparse convolutions (model.py:13-59) --------------
 * The reference runs them through spconv (CUDA only, pyproject.toml:20).  Here: a PLAN per sparsity pattern -- every
 * layer's active sites and its rulebook, built on the device -- and a FORWARD that runs the layers as gathered GEMMs on the
 * fp32 matrix cores with bias and PReLU (model.py:28,37) fused, the last pointwise layer fused with model.py:53-57 (strict
 * upper part zeroed, softplus on the diagonal), L written straight into a lower-triangular CSR with fp64 values -- what
 * dpcg_set_precond_llt takes; test.py:102-105 densifies instead.  Regular sparse convolution, stride 1, windows up to
 * 2 x 2: an output site is active when its window holds an input site; out(y, x) = sum in(y + ky - ph, x + kx - pw) W[ky, kx].
 *   indices: int32 (nnz, 3) rows of (batch, row, col), device, sorted by (batch, row, col) (what data_set.py:122 emits);
 *   kernel_hw / padding_hw: host, 2 ints per layer;  weights[l]: device fp32 (C_out, kh, kw, C_in) -- spconv's KRSC layout;
 *   biases[l] (may be NULL), prelu[l] (device, ONE slope as nn.PReLU(); NULL = no activation after layer l): device fp32. */
typedef struct dpcg_convnet_plan *dpcg_convnet_plan_t;
int dpcg_convnet_plan_create(dpcg_convnet_plan_t *out, int batch, int64_t height, int64_t width, int64_t nnz,
                             const int32_t *indices, int n_layers, const int32_t *kernel_hw, const int32_t *padding_hw,
                             dpcg_stream_t stream);
/* The same for ANOTHER pattern in an existing plan, reusing its device memory (a plan per matrix of a data set then costs
 * no allocations after the first).  On failure the plan is left empty (usable only for another rebuild or destroy). */
int dpcg_convnet_plan_rebuild(dpcg_convnet_plan_t plan, int batch, int64_t height, int64_t width, int64_t nnz,
                              const int32_t *indices, int n_layers, const int32_t *kernel_hw, const int32_t *padding_hw,
                              dpcg_stream_t stream);
int dpcg_convnet_plan_destroy(dpcg_convnet_plan_t plan);
/* active sites and image size after layer `layer`; nnz_lower: entries with col <= row of the LAST layer's sites */
int dpcg_convnet_plan_info(dpcg_convnet_plan_t plan, int layer, int64_t *sites, int64_t *height, int64_t *width,
                           int64_t *nnz_lower);
/* the output sites as (sites, 3) indices sorted by (batch, row, col), and the pattern of the lower-triangular CSR over
 * batch * height rows (sample b = rows [b * height, (b + 1) * height)); device arrays, any may be NULL */
int dpcg_convnet_plan_output(dpcg_convnet_plan_t plan, int32_t *indices_out, int32_t *lower_rowptr, int32_t *lower_col,
                             dpcg_stream_t stream);
/* channels: host, n_layers + 1.  features_in: device fp32 (nnz, channels[0]).  features_out: device fp32 (sites, channels[n])
 * or NULL.  lower_val: device fp64 [nnz_lower] or NULL; lower_softplus = 1 applies model.py:53-57 (both need a pointwise last
 * layer with one output channel).  Enqueues on `stream`; hidden features live in plan-owned buffers. */
int dpcg_convnet_forward(dpcg_convnet_plan_t plan, const int32_t *channels, const float *const *weights,
                         const float *const *biases, const float *const *prelu, const float *features_in,
                         float *features_out, double *lower_val, int lower_softplus, dpcg_stream_t stream);

/* ---- the U-Net variant: PreconditionerSparseUNet (model.py:62-179) ----------------------------------------------------
 * Fixed structure (extras_unet.py states it on torch ops): levels S0 (the input sites) .. S4, each made by a stride-2,
 * padding-1, 3 x 3 convolution of the previous one; 3 x 3 submanifold convolutions on S0 .. S3 (one rulebook per level,
 * shared by the encoder and the decoder layer); inverse convolutions back up through the stride-2 rulebooks read backwards,
 * each followed by LeakyReLU and the skip add of the encoder output on the same level; a pointwise out_conv on S0 with
 * model.py:169-173 applied to every channel.  A PLAN per sparsity pattern holds the levels and rulebooks (built on the device,
 * no sort, no atomics); the FORWARD runs the 17 layers as gathered GEMMs and writes channel 0 of the output into the
 * lower-triangular CSR of S0 (fp64 values).  Invalid sites (outside the image, duplicates) give DPCG_ERR_INVALID; unsorted
 * ones too, with "sorted" in the message.  indices: as for dpcg_convnet_plan_create. */
typedef struct dpcg_unet_plan *dpcg_unet_plan_t;
int dpcg_unet_plan_create(dpcg_unet_plan_t *out, int batch, int64_t height, int64_t width, int64_t nnz,
                          const int32_t *indices, dpcg_stream_t stream);
/* the same for ANOTHER pattern in an existing plan, reusing its device memory; on failure the plan is left empty */
int dpcg_unet_plan_rebuild(dpcg_unet_plan_t plan, int batch, int64_t height, int64_t width, int64_t nnz,
                           const int32_t *indices, dpcg_stream_t stream);
int dpcg_unet_plan_destroy(dpcg_unet_plan_t plan);
/* sites and image size of level `level` (0 .. 4); nnz_lower: entries with col <= row of S0 */
int dpcg_unet_plan_info(dpcg_unet_plan_t plan, int level, int64_t *sites, int64_t *height, int64_t *width, int64_t *nnz_lower);
/* the sites of level `level` as (sites, 3) int32 indices sorted by (batch, row, col), device */
int dpcg_unet_plan_level_indices(dpcg_unet_plan_t plan, int level, int32_t *indices_out, dpcg_stream_t stream);
/* the output sites (= S0, sorted) and the pattern of the lower-triangular CSR over batch * height rows; any may be NULL */
int dpcg_unet_plan_output(dpcg_unet_plan_t plan, int32_t *indices_out, int32_t *lower_rowptr, int32_t *lower_col,
                          dpcg_stream_t stream);
/* channels: host, 6 (c[0] .. c[5] of the module).  Layers in the order enc1 down1 enc2 down2 enc3 down3 enc4 bottleneck up3
 * dec3 up2 dec2 up1 dec1 up0 dec0 out_conv; layer_dims: host, (C_in, C_out) of each layer's weights, checked against
 * `channels`; weights[l]: device fp32 KRSC (C_out, 3, 3, C_in), out_conv (C_out, 1, 1, C_in); biases[l]: device or NULL;
 * slopes: host, the LeakyReLU slope after layers 0 .. 15.  features_in: device fp32 (S0, in_channels).  features_out: device
 * fp32 (S0, c[5]) or NULL; lower_val: device fp64 [nnz_lower] (channel 0) or NULL.  Enqueues on `stream`; no atomics. */
int dpcg_unet_forward(dpcg_unet_plan_t plan, const int32_t *channels, const int32_t *layer_dims, const float *const *weights,
                      const float *const *biases, const float *slopes, const float *features_in, int in_channels,
                      float *features_out, double *lower_val, dpcg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPCG_H */
