/*
 * clrsdp.h -- C ABI of the MI355X-native interior-point step for clustered low-rank SDPs.
 *
 * This is the drop-in boundary for the hot path of nanleij/Clustered-Low-Rank-SDP-solver
 * (MPMP.jl).  The reference has no FFI of its own: its seam is a set of Julia
 * calls inside the `solverank1sdp` loop (MPMP.jl:742-954).  Every entry point below names the
 * reference function(s) it replaces.  A host (the Python mirror in
 * clustered-low-rank-sdp-solver_amd/solver.py, or the Julia `ccall` shim in INTEGRATION.md)
 * keeps `solvempmp` / `prepareabc` / `solverank1sdp` and calls these.
 *
 * Conventions
 *   - plain C types; sizes are int64_t; matrices are column-major.
 *   - multi-word numbers (precision_words w = 2 double-double, 4 quad-double) are passed as
 *     PLANAR limbs: an array of n values is w consecutive planes of n doubles, plane 0 = the
 *     leading (hi) limb.  w = 1 is plain IEEE binary64.
 *   - every call returns an int status (CLRSDP_OK = 0); no exception crosses the ABI; the
 *     message of the last failure is returned by clrsdp_last_error().
 *   - host pointers are borrowed for the duration of a call only; the handle owns all device
 *     memory (constraint data stays resident across iterations).
 *   - calls are synchronous w.r.t. the host, not re-entrant per handle, safe across handles.
 */
#ifndef CLRSDP_H
#define CLRSDP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference's failure outcomes) ---------------------- */
#define CLRSDP_OK 0
#define CLRSDP_E_ARG 1        /* invalid argument / shape                                     */
#define CLRSDP_E_HIP 2        /* HIP runtime failure (no device, out of memory, ...)         */
#define CLRSDP_E_NOT_PD_X 3   /* spd_inv! failed on a block of X      (MPMP.jl:774-797)       */
#define CLRSDP_E_NOT_PD_S 4   /* "S was not decomposed succesfully"   (MPMP.jl:1439)          */
#define CLRSDP_E_NOT_PD_Q 5   /* "Q was not decomposed correctly"     (MPMP.jl:1503)          */
#define CLRSDP_E_STEP 6       /* step length failed: cho!(X or Y)     (MPMP.jl:1846-1882)      */
#define CLRSDP_E_EXCHANGE 7   /* the multi-rank exchange callback failed                     */
#define CLRSDP_E_STATE 8      /* call out of order (e.g. iterate before upload)              */

/* ---- stages of one iteration (MPMP.jl:755-887); clrsdp_iterate runs them in this order ---- */
#define CLRSDP_STAGE_MU_R 0        /* mu = <X,Y>/dim, mu_p, R = mu_p I - XY   (755-761, 1189)   */
#define CLRSDP_STAGE_XINV 1        /* X^-1 per block (spd_inv!)               (762-801)         */
#define CLRSDP_STAGE_SCHUR 2       /* S_j and A_Y        (compute_S_integrated, 1218-1414)      */
#define CLRSDP_STAGE_FACTOR 3      /* chol(S_j), L^-1 B_j, Q, chol(Q)         (1429-1505)       */
#define CLRSDP_STAGE_RESIDUALS 4   /* P, p, d            (compute_residuals, 1107-1144)         */
#define CLRSDP_STAGE_PREDICTOR 5   /* dx, dX, dy, dY     (compute_search_direction, 818)        */
#define CLRSDP_STAGE_CORRECTOR_R 6 /* r, beta_c, mu_c, R = mu_c I - XY - dXdY (832-842, 1203)   */
#define CLRSDP_STAGE_CORRECTOR 7   /* corrector direction                     (846-857)         */
#define CLRSDP_STAGE_STEP 8        /* alpha_p, alpha_d   (compute_step_length, 863-874)         */
#define CLRSDP_STAGE_UPDATE 9      /* x,y,X,Y += alpha d*, new objectives     (877-887, 940-941) */
#define CLRSDP_NUM_STAGES 10

/* Inner buckets of the reference's timing table (MPMP.jl:897-898: "Time inside decomp" and
 * "Time inside search directions", printed at 997-1012) */
#define CLRSDP_INNER_SCHUR 0       /* compute_S_integrated                                       */
#define CLRSDP_INNER_CHOL_S 1      /* factorisation of S_j (Cholesky + L^-1, or approx_lu!)      */
#define CLRSDP_INNER_CINVB 2       /* L_j^-1 B_j (and B_j^T U_j^-1)                               */
#define CLRSDP_INNER_Q 3           /* Q = sum_j W_j^T W_j (+ the exchange)                        */
#define CLRSDP_INNER_CHOL_Q 4      /* factorisation of Q                                          */
#define CLRSDP_INNER_Z 5           /* Z = sym(X^-1 (P Y - R)) and its trace_A products            */
#define CLRSDP_INNER_RHS_X 6       /* rhs_x = -d - Tr(A_* Z)                                      */
#define CLRSDP_INNER_SOLVE 7       /* the block solve for dx, dy                                  */
#define CLRSDP_INNER_DX 8          /* dX = P + sum dx_i A_i                                        */
#define CLRSDP_INNER_DY 9          /* dY = sym(X^-1 (R - dX Y))                                    */
#define CLRSDP_NUM_INNER 10

/* ---- device buffers readable with clrsdp_get_buffer (stage-level parity tests) ----------- */
#define CLRSDP_BUF_X 0        /* block-diagonal state X, blocks concatenated, column-major   */
#define CLRSDP_BUF_Y 1
#define CLRSDP_BUF_XINV 2     /* X^-1 after STAGE_XINV                                       */
#define CLRSDP_BUF_R 3        /* R after STAGE_MU_R / STAGE_CORRECTOR_R                      */
#define CLRSDP_BUF_S 4        /* S_j (full symmetric) after STAGE_SCHUR, clusters concatenated */
#define CLRSDP_BUF_AY 5       /* A_Y: per block, per (r,s) with r>=s, K values               */
#define CLRSDP_BUF_Q 6        /* Q = sum_j B_j^T S_j^-1 B_j before its factorisation           */
#define CLRSDP_BUF_P 7        /* primal residual P (blocks)                                  */
#define CLRSDP_BUF_PVEC 8     /* p (n_y)                                                      */
#define CLRSDP_BUF_DVEC 9     /* d (local sum dim_S)                                           */
#define CLRSDP_BUF_DX 10      /* dx (local)                                                   */
#define CLRSDP_BUF_DXMAT 11   /* dX (blocks)                                                  */
#define CLRSDP_BUF_DY 12      /* dy (n_y)                                                     */
#define CLRSDP_BUF_DYMAT 13   /* dY (blocks)                                                  */
#define CLRSDP_BUF_XVEC 14    /* x (local)                                                    */
#define CLRSDP_BUF_YVEC 15    /* y (n_y)                                                      */
#define CLRSDP_BUF_SCALARS 16 /* clrsdp_scalar slots (see CLRSDP_SC_*)                          */
#define CLRSDP_BUF_LXINV 17   /* STAGE_XINV's factor buffer (blocks): L_X^-1 on the on-chip path */
#define CLRSDP_BUF_LQINV 18   /* chol(Q)'s factor buffer (n_y^2): L_Q^-1 on the on-chip path    */
#define CLRSDP_BUF_QINV 19    /* Q^-1 (n_y^2) where the Q solve uses it (fp64, n_y <= 128)      */
#define CLRSDP_NUM_BUFS 17

/* slots of CLRSDP_BUF_SCALARS */
#define CLRSDP_SC_MU 0
#define CLRSDP_SC_MU_P 1
#define CLRSDP_SC_R 2
#define CLRSDP_SC_BETA 3
#define CLRSDP_SC_BETA_C 4
#define CLRSDP_SC_MU_C 5
#define CLRSDP_SC_ALPHA_P 6
#define CLRSDP_SC_ALPHA_D 7
#define CLRSDP_SC_MINEIG_X 8
#define CLRSDP_SC_MINEIG_Y 9
#define CLRSDP_SC_POBJ 10
#define CLRSDP_SC_DOBJ 11
#define CLRSDP_SC_ERR_P_MAT 12
#define CLRSDP_SC_ERR_P_VEC 13
#define CLRSDP_SC_ERR_D_VEC 14
#define CLRSDP_SC_DOT_XY 15
#define CLRSDP_SC_DOT_XDY 16
#define CLRSDP_NUM_SCALARS 24

/* Problem description: the fields of BlockInfo (MPMP.jl:467-513) the device needs.
 * Global over ALL clusters (every rank passes the same description). */
typedef struct {
  int64_t J;                 /* number of clusters                                          */
  int64_t n_y;               /* number of free variables y                                  */
  const int64_t* m;          /* [J]  polynomial-matrix size m_j                              */
  const int64_t* L;          /* [J]  blocks per cluster                                      */
  const int64_t* n_samples;  /* [J]  N_j                                                     */
  const int64_t* delta;      /* [sum_j L_j] vector length of block (j,l), (j,l) order         */
  const int64_t* ranks;      /* [sum_{j,l} N_j] rank of (j,l,k), (j,l,k) order               */
} clrsdp_desc;

typedef struct {
  int32_t precision_words;   /* 1 = fp64, 2 = double-double, 4 = quad-double                 */
  int32_t device;            /* HIP device ordinal                                            */
  int32_t rank;              /* this process's rank, 0 <= rank < world_size                   */
  int32_t world_size;        /* number of processes (one per GPU)                             */
  const int32_t* owned;      /* clusters owned by this rank (ascending); NULL = all clusters  */
  int32_t n_owned;
  int32_t timing;            /* nonzero: record per-phase HIP events into clrsdp_iter_stats   */
} clrsdp_config;

/* solverank1sdp keyword arguments used inside the loop body (MPMP.jl:599-613); each value is
 * given as up to 4 limbs (unused limbs 0). */
typedef struct {
  double beta_infeasible[4];
  double beta_feasible[4];
  double gamma[4];
  double b0[4];
} clrsdp_params;

/* Loop-control thresholds of terminate() and check_pd_feasibility() (MPMP.jl:606-611,
 * 1147-1185), up to 4 limbs each; used by the pipelined loop (clrsdp_iterate_async). */
typedef struct {
  double duality_gap_threshold[4];
  double primal_error_threshold[4];
  double dual_error_threshold[4];
  int32_t need_primal_feasible;
  int32_t need_dual_feasible;
} clrsdp_control;

/* What one loop body produces for the host's log row and termination test (MPMP.jl:923-953).
 * All values are the leading limb. */
typedef struct {
  double mu;        /* mu at the start of the iteration                           (755)      */
  double P_err;     /* max |P_ij| of the residual computed this iteration         (931)      */
  double p_err;     /* max |p_i|                                                  (932)      */
  double d_err;     /* max |d_i|                                                  (933)      */
  double alpha_p;   /* primal step                                                (934)      */
  double alpha_d;   /* dual step                                                  (935)      */
  double beta_c;    /* corrector beta                                             (936)      */
  double p_obj;     /* <c,x> + b0 after the update                                (940)      */
  double d_obj;     /* <C,Y> + <b,y> + b0 after the update                        (941)      */
  double phase_ms[CLRSDP_NUM_STAGES]; /* per-stage device time when config.timing != 0       */
  int32_t status;
  /* timing mode 1 only: the reference's inner timings (MPMP.jl:897-898, 997-1012), device time
   * of the launches of each bucket (side-stream work included, measured on its own stream):
   * CLRSDP_INNER_* below; the direction buckets are predictor + corrector */
  double inner_ms[CLRSDP_NUM_INNER];
  /* the loop control of the state after this body at the word's full width (up to 4 limbs, hi
   * first; unused limbs 0): the duality gap (MPMP.jl:942; for clrsdp_initial_residuals the gap
   * without b0, 725) and the errors of the residuals computed in this body (943-944), as the
   * device's terminate()/check_pd_feasibility() compares them (1147-1185) */
  double gap_w[4];
  double P_err_w[4];
  double p_err_w[4];
  double d_err_w[4];
} clrsdp_iter_stats;

/* Multi-rank exchange: gather `bytes` bytes from `send_dev` on every rank into `recv_dev`
 * (rank r's bytes at offset r*bytes).  send_dev/recv_dev are the device buffers registered
 * with clrsdp_set_exchange.  Called on the host, in the middle of a stage, with the library's
 * work on `stream` enqueued but not necessarily finished; the callee must order its transfer
 * after that work and before anything enqueued later on `stream`.  Return 0 on success. */
typedef int (*clrsdp_exchange_fn)(void* ctx, int32_t tag, int64_t bytes, void* stream);

typedef struct clrsdp_handle clrsdp_handle;

int32_t clrsdp_version(void);
const char* clrsdp_last_error(const clrsdp_handle* h);  /* h may be NULL: last global error */

/* Allocate device state for the clusters owned by this rank.
 * Replaces: the allocations of solverank1sdp (MPMP.jl:660-721) and BlockInfo (MPMP.jl:480). */
int32_t clrsdp_create(const clrsdp_desc* desc, const clrsdp_config* cfg, clrsdp_handle** out);

/* Copy the constraint data (the (A, B, c, H) tuples of prepareabc, MPMP.jl:385-406).
 *  V:      per (j,l) the delta_jl x K_jl matrix of all vectors v_{j,l,k,rnk} (columns in (k,rnk)
 *          order, MPMP.jl:1249-1254), all (j,l) concatenated: sum delta_jl*K_jl values.
 *  lambda: per (j,l) the K_jl eigenvalues H[l,k][rnk], concatenated.
 *  B:      per j the dim_S_j x n_y matrix, concatenated.   c: per j dim_S_j values.
 *  b:      n_y values.   C: NULL (C = 0, MPMP.jl:691-695) or the blocks of C concatenated.
 * Each array is w planes (see conventions); data of clusters not owned is skipped. */
int32_t clrsdp_upload_constraints(clrsdp_handle* h, const double* V, const double* lambda,
                                  const double* B, const double* c, const double* b,
                                  const double* C);

/* State (x, X, y, Y) in the global layout: x has sum_j dim_S_j entries, X and Y all blocks
 * concatenated (column-major), y has n_y.  set: the owned parts are read.  get: the owned
 * parts of x/X/Y are written (others untouched); y is replicated.
 * Replaces: initial_solutions / the returned state (MPMP.jl:613, 660-690, 1014-1024). */
int32_t clrsdp_set_state(clrsdp_handle* h, const double* x, const double* X, const double* y,
                         const double* Y);
int32_t clrsdp_get_state(clrsdp_handle* h, double* x, double* X, double* y, double* Y);

/* Residuals, errors and objectives at the current state, before the loop (MPMP.jl:723-736):
 * fills P_err, p_err, d_err, p_obj, d_obj (with b0) of `st`. */
int32_t clrsdp_initial_residuals(clrsdp_handle* h, const clrsdp_params* prm,
                                 clrsdp_iter_stats* st);

/* One full loop body (MPMP.jl:755-887 + the objective update 940-941).  pd_feas is the host's
 * check_pd_feasibility result from the previous iteration (MPMP.jl:949-953). */
int32_t clrsdp_iterate(clrsdp_handle* h, const clrsdp_params* prm, int32_t pd_feas,
                       clrsdp_iter_stats* st);

/* Pipelined loop (replaces the same loop, MPMP.jl:743-954, with the host one body behind):
 * clrsdp_set_control sets the thresholds; clrsdp_iterate_async enqueues one loop body whose
 * pd_feas and termination are decided on the device from the previous body's results
 * (after clrsdp_initial_residuals for the first) and returns at once; clrsdp_iterate_wait
 * waits for the oldest body in flight and returns its log row.  At most two bodies are in
 * flight.  A body enqueued after the device decided to terminate applies nothing and returns
 * *ran = 0; P, p, d (clrsdp_get_buffer) are then those of the last body that ran. */
int32_t clrsdp_set_control(clrsdp_handle* h, const clrsdp_control* ctl);
int32_t clrsdp_iterate_async(clrsdp_handle* h, const clrsdp_params* prm);
int32_t clrsdp_iterate_wait(clrsdp_handle* h, clrsdp_iter_stats* st, int32_t* ran);

/* Run one stage (CLRSDP_STAGE_*) only; stages must be run in order within an iteration. */
int32_t clrsdp_run_stage(clrsdp_handle* h, int32_t stage, const clrsdp_params* prm,
                         int32_t pd_feas);

/* Read a device buffer (CLRSDP_BUF_*) as w planes of doubles.  *count receives the number of
 * values per plane; host may be NULL to query the size. */
int32_t clrsdp_get_buffer(clrsdp_handle* h, int32_t buf, double* host, int64_t* count);

/* Register the multi-rank exchange (required when world_size > 1).  send_dev / recv_dev are
 * device buffers of at least clrsdp_exchange_bytes() and world_size times that. */
int32_t clrsdp_exchange_bytes(const clrsdp_handle* h, int64_t* bytes);
int32_t clrsdp_set_exchange(clrsdp_handle* h, clrsdp_exchange_fn fn, void* ctx, void* send_dev,
                            void* recv_dev);

/* Native RCCL exchange (the per-cluster partials all-gathered over xGMI, SURVEY.md §8e;
 * replaces the reference's shared-memory reductions across cluster threads, e.g. the Q sum
 * MPMP.jl:1486-1494 and the dy partials 1758-1761).  Rank 0 calls clrsdp_comm_unique_id and
 * hands the CLRSDP_COMM_ID_BYTES bytes to every rank (any host channel); every rank then calls
 * clrsdp_comm_init with them.  The handle creates an RCCL communicator of world_size ranks on
 * its device (RCCL is loaded at run time) and from then on issues every exchange itself as an
 * ncclAllGather on its stream; the exchange callback is no longer used.  With world_size > 1
 * the loop body is enqueued eagerly (the pipelined loop hides the enqueue), or replayed as one
 * hipGraph with the all-gathers captured in it when CLRSDP_GRAPH_RCCL is set.  With
 * world_size 1 the all-gathers are still issued (in place, one rank) inside the graph, which
 * exercises the capture path. */
#define CLRSDP_COMM_ID_BYTES 128
int32_t clrsdp_comm_unique_id(uint8_t* id);
int32_t clrsdp_comm_init(clrsdp_handle* h, const uint8_t* id);

/* Device-side snapshot of the iterate: clrsdp_save_state copies x, X, y, Y and the scalar
 * slots into a buffer of the handle, clrsdp_restore_state copies them back; both are enqueued
 * on the handle's stream (no host synchronisation), so a benchmark can replay a window of loop
 * bodies indefinitely without converging into the fp64 breakdown regime.  (No reference
 * counterpart; initial_solutions, MPMP.jl:613, restarts from the host.) */
int32_t clrsdp_save_state(clrsdp_handle* h);
int32_t clrsdp_restore_state(clrsdp_handle* h);

/* Hand the iterate of one handle to another: x, X, y, Y of `src` are copied into `dst`, device
 * to device (one kernel launch, no host staging).  The two handles may differ in
 * precision_words, which is what the call is for: a solve can run at fp64 while that is good
 * enough and continue at double-double or quad-double from the same iterate
 * (solve_escalating).  Conversion per number, limbs moved as doubles without arithmetic:
 *   dst as wide as src   a bitwise copy
 *   dst wider            the source limbs followed by exact zeros (the same value)
 *   dst narrower         the leading limbs; the library keeps its words renormalised
 *                        (non-overlapping), so this is the value rounded to the narrower width
 *                        (to nearest, up to the usual last-limb ambiguity of a renormalised sum)
 * Ordering: the copy runs after the work already enqueued on src's stream and before anything
 * enqueued later on dst's stream.  The call synchronises both streams (it is not meant for the
 * loop's path), so src may be destroyed as soon as it returns.
 * Afterwards dst is exactly as after clrsdp_set_state with the same values: the <X,Y> partials
 * are refreshed and the next CORRECTOR_R sums its dot product itself; dst's buffers do not move,
 * so its captured loop-body graphs stay valid; its scalar slots, constraints, control and
 * factorisation flags are untouched (call clrsdp_initial_residuals next, as after set_state).
 * Refusals copy nothing and change neither handle's state (clrsdp_last_error(dst) says why):
 *   CLRSDP_E_ARG    a NULL handle; dst == src; different devices; different clrsdp_desc
 *                   contents (J, n_y, m, L, n_samples, delta, ranks); different rank,
 *                   world_size or owned set
 *   CLRSDP_E_STATE  either handle has loop bodies in flight (clrsdp_iterate_async without its
 *                   clrsdp_iterate_wait); src never had a state (clrsdp_set_state or a hand-off)
 * A loop body that failed (CLRSDP_E_NOT_PD_X / _S / _Q, CLRSDP_E_STEP) applied no update, so src
 * then still holds the state from before that body and can hand it over.
 * (No reference counterpart: the reference runs one precision per solve.) */
int32_t clrsdp_handoff_state(clrsdp_handle* dst, clrsdp_handle* src);

/* Run all work on `stream` (a hipStream_t; NULL = the handle's own stream). */
int32_t clrsdp_set_stream(clrsdp_handle* h, void* stream);
void* clrsdp_get_stream(const clrsdp_handle* h);
int32_t clrsdp_synchronize(clrsdp_handle* h);

/* Per-stage HIP-event timing (clrsdp_iter_stats.phase_ms): 0 = off, 1 = every stage (the loop
 * body is enqueued stage by stage, no graph), 2 = only phase_ms[CLRSDP_STAGE_SCHUR]: the sum of
 * the three Schur launches' first-workgroup-start..last-workgroup-end on the 100 MHz device clock,
 * stamped by the kernels inside the replayed loop-body graph (fp64 fast path; 0 elsewhere).
 * With timing 0 or 2 and world_size 1 (or a
 * native RCCL communicator), clrsdp_iterate replays a captured hipGraph of the loop body. */
int32_t clrsdp_set_timing(clrsdp_handle* h, int32_t on);

/* Loop-body hipGraph replay on (default) or off (on = 0: every body is enqueued eagerly from the
 * host, launch by launch, as the sharded path without CLRSDP_GRAPH_RCCL does; a measurement
 * switch, e.g. for the host enqueue time of one body).  No reference counterpart. */
int32_t clrsdp_set_graph(clrsdp_handle* h, int32_t on);

/* The exchange this handle's loop body uses: *backend 0 = none (one rank),
 * 1 = the native RCCL communicator of clrsdp_comm_init (*nranks = ncclCommCount of it),
 * 2 = the clrsdp_set_exchange callback (*nranks = world_size).  Replaces nothing in the
 * reference (shared-memory threads, MPMP.jl:1486-1494, 1758-1761). */
int32_t clrsdp_comm_info(const clrsdp_handle* h, int32_t* nranks, int32_t* backend);

/* What this handle's SCHUR stage launches (read-only; adds no switch and no launch).  The plan is
 * fixed by clrsdp_create / clrsdp_upload_constraints from the block shapes, the ranks and the
 * CLRSDP_SCHUR_* / CLRSDP_OZAKI / CLRSDP_MW_PAIR_UPPER environment at that time:
 *   fast        fp64 and every local block m = 1: the V^T X^-1 / V^T Y products and the pairing
 *               kernels below (0: the general path, four GEMMs or the int8 products, extract_AY
 *               and schur_assemble)
 *   fused       schur_fused_f64 runs (0 with fast: the V^T X^-1 GEMM + schur_pairs_f64)
 *   one, d64    its one-column-tile-per-workgroup form, and that form's delta <= 64 instance
 *   grp2        fused: the rank-2 group-sum epilogue instance; unfused: some cluster has its
 *               2 x 2 groups summed by schur_pairs_f64 (per descriptor)
 *   fused_y     V^T Y formed on chip by the fused kernel (0: read from the GEMM's output)
 *   n_fwg       workgroups of the fused launch (0 when it does not run)
 *   n_ptiles    workgroups of schur_pairs_f64, were it to run (fast only)
 *   n_gsum      clusters summed from the G arena by schur_gsum (L > 1 or mixed ranks)
 *   ozaki       the int8 (oz_split / oz_gemm) products (double-double, every block m = 1)
 *   pair_upper  multi-word, every m = 1: BX / BY hold their upper 16-tiles only
 *   full        of the last SCHUR enqueued: 1 = both triangles of every S_j were stored by the
 *               kernels (always so without the fused kernel: schur_pairs_f64, schur_gsum and
 *               schur_assemble store both), 0 = the fused kernel was told to store the lower
 *               one; -1 before any
 *   s_lower     BUF_S holds the lower triangle only (clrsdp_get_buffer mirrors it on the host);
 *               0 again once FACTOR has overwritten S; -1 before any SCHUR
 * No reference counterpart (compute_S_integrated, MPMP.jl:1373-1398, is one loop nest). */
struct clrsdp_schur_info {  /* (a tag only: the function below has the same name) */
  int32_t fast, fused, one, d64, grp2, fused_y;
  int32_t n_fwg, n_ptiles, n_gsum;
  int32_t ozaki, pair_upper;
  int32_t full, s_lower;
};
int32_t clrsdp_schur_info(const clrsdp_handle* h, struct clrsdp_schur_info* out);

/* Factorisations of S_j, Q and X (flags, default CLRSDP_FACT_FALLBACK).  The device factorises
 * S_j and Q by Cholesky (they are SPD) and X^-1 by the Cholesky inverse (spd_inv!).  The
 * reference factorises S_j and Q by partially pivoted LU (approx_lu!, MPMP.jl:1433-1442,
 * 1499-1505) and switches X^-1 to LU when spd_inv! fails (approx_inv!, MPMP.jl:774-786):
 *   CLRSDP_FACT_FALLBACK  when a Cholesky fails, set the matching LU flag and re-run the loop
 *                         body (its update was not applied); LU then stays on for the solve
 *   CLRSDP_FACT_LU_SQ     S_j and Q by pivoted LU now (the reference's own factorisation)
 *   CLRSDP_FACT_LU_X      X^-1 by pivoted LU now (approx_inv!)
 * clrsdp_get_factorization reports the current flags (a fallback adds its LU flag).
 * A failed LU is the reference's error (CLRSDP_E_NOT_PD_S / _Q / _X). */
#define CLRSDP_FACT_FALLBACK 1
#define CLRSDP_FACT_LU_SQ 2
#define CLRSDP_FACT_LU_X 4
int32_t clrsdp_set_factorization(clrsdp_handle* h, int32_t flags);
int32_t clrsdp_get_factorization(const clrsdp_handle* h, int32_t* flags);
int32_t clrsdp_destroy(clrsdp_handle* h);

/* Stand-alone step length of a block-diagonal pair, fp64 (replaces compute_step_length,
 * MPMP.jl:1829-1898, without a handle): M_b = L_b L_b^T and lambda_b = lambda_min(L_b^-1 dM_b
 * L_b^-T) per block, then *alpha = 1 if min_b lambda_b > -gamma, else -gamma / min_b lambda_b
 * (1893-1897).  The nblocks blocks of sizes n[] are concatenated column-major in M and dM (host
 * memory); min_eig (may be NULL) receives the nblocks lambda_b.  CLRSDP_E_STEP when some M_b is
 * not positive definite (cho! fails, 1846-1848 / 1882). */
int32_t clrsdp_step_length(int32_t device, int64_t nblocks, const int64_t* n, const double* M,
                           const double* dM, double gamma, double* alpha, double* min_eig);

/* lambda_min of each symmetric block at fp64 (words 1), double-double (2) or quad-double (4):
 * the eigenvalue part of compute_step_length (MPMP.jl:1857-1870, approx_eig_qr! of L^-1 dM L^-T),
 * Householder tridiagonalisation + Sturm multisection (+ the multi-word Newton tail) as the
 * loop body runs it.  A: the nblocks blocks of sizes n[] concatenated column-major, as `words`
 * planes of doubles (hi limb first; the blocks must be exactly symmetric); min_eig: `words` planes of nblocks values.
 * 1 <= n[b] <= 4096.  Scale: each block is divided by the power of two of its largest leading-limb
 * magnitude on load and lambda_min multiplied back (exact), so the result is relative to the
 * block's norm at any scale; supported (and tested) for blocks whose largest |entry| lies in
 * [2^-600, 2^600].  Outside it the trailing limbs of a multi-word entry or of the result can
 * fall into the subnormal range and the accuracy degrades towards fp64's.
 *
 * The kernel is chosen by the word width and the largest block of the call (nmax);
 * clrsdp_eigmin_kernel reports it:
 *   words | kernel by nmax
 *   1     | eigmin_split <= 128; eigmin_lds 129-138; eigmin_batched >= 139
 *   2     | eigmin_mx (+ eigmin_lds2 for the blocks it cannot certify) <= 64; eigmin_lds2 65-93;
 *         | eigmin_lds 94-96; eigmin_batched >= 97
 *   4     | eigmin_mx (+ eigmin_lds2) <= 64; eigmin_lds 65-66; eigmin_batched >= 67
 * (CLRSDP_EIG_MX=0: eigmin_lds2 in eigmin_mx's range.)
 * Size bound of the default: eigmin_batched is one workgroup per block and asks for
 * sizeof(word) (4 nmax + 256) bytes of dynamic LDS and never sets the kernel's
 * max-dynamic-LDS attribute.  By reading, not by running: the request passes 64 KiB (HIP's
 * documented limit without the attribute) beyond nmax = 1984 (fp64), 960 (double-double) and 448
 * (quad-double), and the 160 KiB of a CU -- which is what hipFuncGetAttributes reports as the
 * kernel's limit on an MI355X -- beyond 5056, 2496 and 1216.  The default has not been run past
 * the first figures; past the second the runtime refuses the launch (CLRSDP_E_HIP).
 * CLRSDP_EIG_BLK=1 (environment, read when the call builds its plan; default off) sends every
 * batch of eigmin_batched's range to the eigblk_* chain instead: the tridiagonalisation runs
 * across workgroups with one launch per column, the multisection of eigmin_lds follows, and
 * lambda_min of a block is bitwise independent of the rest of the batch.  Its bound is the two
 * on-chip vectors of a column step, 2 nmax words in 160 KiB: beyond this entry point's 4096 at
 * fp64 and double-double, nmax <= 2560 at quad-double (larger: CLRSDP_E_ARG).
 * CLRSDP_EIG_MX_BLK=1 (environment, read when the call builds its plan; default off, and off
 * with CLRSDP_EIG_MX=0) sends every multi-word batch of eigmin_batched's range through the
 * mxblk_* route first, eigmin_mx's scheme across workgroups: the fp64 eigblk_* chain on the
 * leading limbs, an fp64 Cholesky factor of A_h - mu I as the correction operator, and a few
 * refinement steps at the word's width (one n^2 matrix-vector product each), accepted by
 * Temple's bound.  The blocks it cannot certify (a multiple or tightly clustered lambda_min,
 * n < 3) are flagged and go to the route the switch replaced -- eigmin_batched, or the
 * multi-word chain with CLRSDP_EIG_BLK=1 or where eigmin_batched's request passes 64 KiB --
 * in a second, flagged launch.  fp64 batches never take it. */
int32_t clrsdp_eigmin(int32_t device, int32_t words, int64_t nblocks, const int64_t* n,
                      const double* A, double* min_eig);

/* clrsdp_eigmin plus, per block, how lambda_min was obtained: route[b] = 0 certified by the
 * refinement step of the batch's kernel (eigmin_mx, the mxblk_* route); 1 flagged by it and
 * computed by the fallback launch; -1 the batch's kernel has no certification step. */
int32_t clrsdp_eigmin_routes(int32_t device, int32_t words, int64_t nblocks, const int64_t* n,
                             const double* A, double* min_eig, int32_t* route);

/* Which kernel clrsdp_eigmin (and the STEP stage's eigen launches) takes for a batch at `words`
 * whose largest block is nmax (1 .. 4096), under the current environment.  A host-only query:
 * no device is touched and nothing is launched. */
#define CLRSDP_EIG_K_SPLIT 0    /* eigmin_split (fp64, matrix in registers)                  */
#define CLRSDP_EIG_K_MX 1       /* eigmin_mx, then eigmin_lds2 on the flagged blocks         */
#define CLRSDP_EIG_K_LDS2 2     /* eigmin_lds2                                               */
#define CLRSDP_EIG_K_LDS 3      /* eigmin_lds                                                */
#define CLRSDP_EIG_K_BATCHED 4  /* eigmin_batched (one workgroup per block, global memory)   */
#define CLRSDP_EIG_K_BLK 5      /* eigblk_* chain across workgroups (CLRSDP_EIG_BLK=1)       */
#define CLRSDP_EIG_K_MXBLK 6    /* mxblk_* route, then the flagged blocks (CLRSDP_EIG_MX_BLK=1) */
int32_t clrsdp_eigmin_kernel(int32_t words, int64_t nmax, int32_t* kernel);

/* Partially pivoted LU of each block in place, A_b[perm_b] = L_b U_b (approx_lu!, MPMP.jl:1436,
 * 1501; the factor of approx_inv!, 781), as the solver's LU path runs it.  A: nblocks blocks of
 * sizes n[] concatenated column-major as `words` planes; on return L (unit, below the diagonal)
 * and U.  perm: sum n[] entries, perm_b[k] = original row at position k (0-based).  info: nblocks,
 * 0 or the 1-based column of the first zero pivot. */
int32_t clrsdp_getrf(int32_t device, int32_t words, int64_t nblocks, const int64_t* n,
                     double* A, int32_t* perm, int32_t* info);

/* Cholesky factorisation of each symmetric positive definite block, A_b = L_b L_b^T (cho!,
 * MPMP.jl:1433-1442, 1499-1505, 1846), by the kernels the loop body runs.  A: nblocks blocks of
 * sizes n[] (1 <= n[b] <= 4096) concatenated column-major as `words` planes (1, 2 or 4; hi limb
 * first).  Only the lower triangle of a block is used: whatever stands above the diagonal on
 * entry, NaN included, does not change the result.
 *   inverse = 0: in place through the solver's potrf plan.  On return the lower triangle holds
 *     L_b; the strict upper triangle is unspecified (potrf_batched leaves the input there, the
 *     other kernels write zeros).  fp64: potrf_batched at every n; double-double: chol_lookahead
 *     up to 64 and the potrf_blk_* chain across workgroups beyond (CLRSDP_POTRF_BLK=0:
 *     chol_lookahead up to 128, potrf_batched beyond); quad-double: chol_lookahead (LDL form) up
 *     to 64, potrf_batched beyond.  potrf_batched keeps a 16-column panel of the matrix on chip:
 *     past the n at which it fits (fp64 1262, quad-double 302, double-double 622) the call is
 *     CLRSDP_E_ARG, as the loop body's Cholesky of such a block is (clrsdp_iterate,
 *     clrsdp_run_stage; with CLRSDP_FACT_LU_SQ the body factors it by pivoted LU instead).
 *     CLRSDP_POTRF_BLK is three-state: unset and 0 as above (the default and its refusals are
 *     unchanged); set to anything that does not start with 0, a blocked chain across workgroups
 *     replaces potrf_batched at every word type -- fp64: potrf64_first / _trsm / _update at
 *     every n (16-column panels, the panel by substitution, the trailing update on the fp64
 *     matrix cores; zeros above the diagonal); quad-double: chol_lookahead up to 64, the
 *     potrf_blk_* chain (LDL diagonal step) beyond; double-double as above -- and then no
 *     Cholesky is refused for its size, here (n up to 4096) or in a handle's FACTOR stage.
 *   inverse = 1: A receives L_b^-1 (chol_inv_tiles at fp64, n[b] <= 256; chol_lookahead with
 *     the inverse at double-double and quad-double, n[b] <= 64; larger: CLRSDP_E_ARG).  The
 *     lower triangle holds L_b^-1 and the strict upper triangle exact zeros, every entry written
 *     by the kernel.
 * info: nblocks values, 0 or the 1-based column of the first pivot that is not positive (NaN
 * included); at fp64 with inverse = 1 the first column of the 16-column diagonal tile that holds
 * it.  After a failure that block's contents are unspecified; the other blocks are complete. */
int32_t clrsdp_potrf(int32_t device, int32_t words, int32_t inverse, int64_t nblocks,
                     const int64_t* n, double* A, int32_t* info);

/* Which kernel clrsdp_potrf with inverse = 0 (and the FACTOR stage's Cholesky launches) takes for
 * a batch at `words` whose largest block is nmax (1 .. 4096), under the current environment
 * (CLRSDP_POTRF_BLK).  A host-only query: no device is touched and nothing is launched.  It
 * answers the route, not potrf_batched's size refusal, which needs the kernel's static LDS from
 * the code object and so a device. */
#define CLRSDP_POTRF_K_BATCHED 0  /* potrf_batched (one workgroup per block, 16-column panels)    */
#define CLRSDP_POTRF_K_LA64 1     /* chol_lookahead<.., 64, 15, true>; the LDL form at quad-double */
#define CLRSDP_POTRF_K_LA128 2    /* chol_lookahead<.., 128> (double-double only)                 */
#define CLRSDP_POTRF_K_BLK 3      /* potrf_blk_* chain across workgroups (multi-word)             */
#define CLRSDP_POTRF_K_BLK64 4    /* potrf64_* chain across workgroups (fp64)                     */
int32_t clrsdp_potrf_kernel(int32_t words, int64_t nmax, int32_t* kernel);

/* L_b^-1 and, for the blocks that ask, A_b^-1 = L_b^-T L_b^-1 of fp64 symmetric positive definite
 * blocks in ONE launch of the form of chol_inv_tiles that keeps the tiles of A^-1 in its
 * accumulators (the XINV stage's launch, and chol(Q)'s).  A: nblocks blocks of sizes n[]
 * (1 <= n[b] <= 128) concatenated column-major, pitch n[b]; only lower triangles are read.
 * Linv and Ainv: block b is n[b] columns of pitch ld[b] >= n[b] (ld null: pitch n[b]), blocks
 * concatenated; both are copied to the device before the launch and back after it, so an entry
 * the kernel does not write returns as it came.  Linv_b receives L_b^-1 (exact zeros above the
 * diagonal), the same bits whether or not A_b^-1 is asked for.  want[b] != 0: Ainv_b receives
 * the full, exactly symmetric A_b^-1; want[b] = 0, or a block that fails: Ainv_b is not written
 * (want null: no block asks, Ainv may be null).  Rows past n[b] of a column are never written.
 * info as clrsdp_potrf with inverse = 1. */
int32_t clrsdp_chol_spdinv(int32_t device, int64_t nblocks, const int64_t* n, const int64_t* ld,
                           const int32_t* want, const double* A, double* Linv, double* Ainv,
                           int32_t* info);

/* Whether a batch of on-chip factorisations with the inverse whose largest block is nmax, at
 * `words`, takes that form (*fused = 1) or the plain one with the product L^-T L^-1 as a GEMM
 * behind it (0), under the current environment (CLRSDP_CHOL_SPDINV): fp64 and nmax <= 128 only,
 * and never when the inverse comes from the pivoted LU (lu != 0: CLRSDP_FACT_LU_X for X,
 * CLRSDP_FACT_LU_SQ for Q).  A host-only query: no device is touched. */
int32_t clrsdp_spdinv_kernel(int32_t words, int64_t nmax, int32_t lu, int32_t* fused);

/* Triangular solves of each block in place on B_b (n[b] x nrhs[b]), as the solver runs them
 * (approx_solve_tril! / approx_solve_triu!, MPMP.jl:1457-1460, 1751-1773): trsm_batched (the
 * one-wave vector kernels for multi-word mode 0 blocks of n <= 128) wherever its on-chip panel
 * fits, the blocked chain across workgroups beyond.  mode 0: A_b holds a lower triangular L
 * (potrf's; the strict upper triangle is not read); mode 1: the unit lower L of clrsdp_getrf's
 * factors (only the strict lower triangle is read); mode 2: their U, read transposed.  trans = 0
 * solves L x = b (mode 2: U^T x = b), trans != 0 solves L^T x = b (mode 2: U x = b).  A: nblocks
 * blocks of sizes n[] concatenated column-major as `words` planes; B likewise, block b with
 * leading dimension n[b].  1 <= n[b], nrhs[b] <= 4096. */
int32_t clrsdp_trsm(int32_t device, int32_t words, int32_t mode, int32_t trans,
                    int64_t nblocks, const int64_t* n, const int64_t* nrhs,
                    const double* A, double* B);

/* One batched product launch, C_p = alpha op(A_p) op(B_p) + beta C_in,p (+ dmult * *dscal on the
 * diagonal), through the solver's own GemmPlan (the products of every stage: X^-1, R, the Schur
 * pairings V^T X^-1 V, W_j, Q, the weighted A, the directions), at fp64 (words 1), double-double
 * (2) or quad-double (4).  The plan is built from the records below exactly as build_plans()
 * builds the solver's, finalised and launched once on a stream of the call's own; *path (may be
 * NULL) receives the kernel that the plan's launch selected.
 *
 * Buffers.  A, B, C, C_in, and sa / sl are arenas of na, nb, nc, ncin and ns numbers, each as
 * `words` planes (hi limb first).  Problem p's operands start at the element offsets offa, offb,
 * offc, offcin (and offs into sa and sl) and are column-major with the leading dimensions lda,
 * ldb, ldc, ldcin.  Stored shapes: A is M x K (transa: K x M), B is K x N (transb: N x K), C and
 * C_in are M x N; every leading dimension is at least the stored row count and at most 2^24.  A
 * and B are read only inside the stored rows (rows between the row count and the leading
 * dimension are never loaded).  The whole C arena is copied to the device before the launch and
 * back after it, so whatever the caller puts into the padding rows, the gaps between problems and
 * the ends of the arena comes back bitwise unless a kernel wrote there.  The C regions of two
 * problems (offc .. offc + (N - 1) ldc + M) must not overlap.  The offsets decide the kernel at
 * fp64: equal shapes, leading dimensions and constant offset differences in every arena make a
 * uniform batch (gemm_f64_uni), anything else goes through descriptors (gemm_f64_lds).
 *
 * C_in.  beta = 0: C_in is not read.  Otherwise problem p reads C_in at offcin, or, when the
 * C_in arena is NULL or the problem's offcin is negative, its own C in place (ldcin is then
 * ignored), as R -= dX dY does.
 *
 * form
 *   CLRSDP_GEMM_PLAIN   GemmPlan::add.
 *   CLRSDP_GEMM_SYM     add with sym = true (fp64, square, op(A) = A, beta = 0, no dscal): the
 *                       product is symmetric in exact arithmetic (L^-1 dM L^-T); only the lower
 *                       tiles are computed, each is written with its mirror image and a diagonal
 *                       tile mirrors its lower triangle, so C is exactly symmetric.
 *   CLRSDP_GEMM_UPPER   add with upper = true (multi-word, square): only the 8 x 8 tiles on and
 *                       above the diagonal are computed; tiles strictly below it are not written.
 *   CLRSDP_GEMM_SCALED  add_scaled (fp64, transa = 0, transb = 1): op(A) = A diag(sa .* sl), the
 *                       K factors of problem p at sa + offs, sl + offs.
 *   CLRSDP_GEMM_MIXED   add_op (fp64): transa, transb, alpha and beta are each record's own (the
 *                       call's are ignored); a record with diag != 0 (square) adds *dscal, once,
 *                       to its diagonal (the kernel's flags bit 4; dmult is ignored).
 * dscal (may be NULL; fp64 only): one number in host memory; PLAIN and SCALED add dmult * *dscal
 * to C(i, i) of every problem (GemmPlan::launch's dscal, as R = mu I - X Y uses it).  Not with a
 * batch that takes the GEMV kernel.
 *
 * *path: the kernel, derived by GemmPlan::path() from the fields launch() branches on.  A batch
 * whose problems all have N = 1 (and, with transb, K = 1) takes gemv_batched, one of its five
 * code paths; a MIXED or SCALED batch never does. */
#define CLRSDP_GEMM_PLAIN 0
#define CLRSDP_GEMM_SYM 1
#define CLRSDP_GEMM_UPPER 2
#define CLRSDP_GEMM_SCALED 3
#define CLRSDP_GEMM_MIXED 4

#define CLRSDP_PATH_GEMV_N_F64 1  /* gemv_batched fp64, op(A) = A: 32 loads in flight, 128-k steps */
#define CLRSDP_PATH_GEMV_T_F64 2  /* gemv_batched fp64, op(A) = A^T: 16-lane sums, 128 / 32 / 16 k */
#define CLRSDP_PATH_GEMV_N_MW 3   /* gemv_batched multi-word, op(A) = A: 32-k steps, then 4         */
#define CLRSDP_PATH_GEMV_T_QD 4   /* gemv_batched quad-double A^T: thread per column ("deep")       */
#define CLRSDP_PATH_GEMV_T_DD 5   /* gemv_batched double-double A^T: the 16-lane reduction           */
#define CLRSDP_PATH_UNI64 6       /* gemm_f64_uni, 64 x 64 tiles                                     */
#define CLRSDP_PATH_UNI32 7       /* gemm_f64_uni, 32 x 32 tiles (CLRSDP_GEMM_TS32_BELOW)            */
#define CLRSDP_PATH_LDS 8         /* gemm_f64_lds (descriptors; 64 x 64 tiles)                       */
#define CLRSDP_PATH_DYN 9         /* gemm_f64_dyn (MIXED)                                            */
#define CLRSDP_PATH_VALU_KS 10    /* gemm_valu_ks (multi-word, 8 x 8 tiles)                          */

typedef struct {
  int64_t M, N, K;                   /* 1 .. 4096 each                                          */
  int64_t lda, ldb, ldc, ldcin;
  int64_t offa, offb, offc, offcin;  /* element offsets into the arenas; offcin < 0: in place    */
  int64_t offs;                      /* SCALED: offset of the K factors in sa and sl             */
  int32_t transa, transb, diag;      /* MIXED only                                               */
  int32_t reserved;
  double alpha, beta;                /* MIXED only                                               */
} clrsdp_gemm_problem;

/* Refused with CLRSDP_E_ARG before any device work: a NULL prob, A, B or C; nprob outside
 * 1 .. 65536; M, N or K outside 1 .. 4096 (K = 0 in particular: the tiled kernels clamp their
 * loads to index K - 1); a leading dimension below its stored row count; SYM or UPPER on a
 * non-square problem; SYM, SCALED, MIXED or dscal with words != 1; UPPER with words = 1; SCALED
 * other than transa = 0, transb = 1, or without sa and sl; SYM with transa, beta != 0 or dscal;
 * a diag record that is not square or comes without dscal; an operand that does not lie inside
 * its arena; overlapping C regions. */
int32_t clrsdp_gemm(int32_t device, int32_t words, int32_t form, int32_t transa, int32_t transb,
                    double alpha, double beta, const double* dscal, double dmult, int64_t nprob,
                    const clrsdp_gemm_problem* prob, const double* A, int64_t na, const double* B,
                    int64_t nb, double* C, int64_t nc, const double* Cin, int64_t ncin,
                    const double* sa, const double* sl, int64_t ns, int32_t* path);

/* One chain_f64 launch through the solver's ChainPlan: fp64, nprob blocks of n x n (1 <= n <= 128)
 * per pointer set, block p of every array at element offset p n^2, leading dimension n.
 *   CLRSDP_CHAIN        O_p = A2_p (a1 A1_p B1_p + b1 C1_p); C1 may be NULL (no second term).
 *                       Z = X^-1 (P Y - R) is (a1, b1) = (1, -1), dY = X^-1 (R - dX Y) is (-1, 1).
 *                       With dot_part != NULL (then DA, DdA, DB are required, nprob n^2 each) the
 *                       launch also leaves the raw per-workgroup partial sums of
 *                       <DA + DdA, DB + O>: nprob * ceil(n / 32) numbers, workgroup b (strip
 *                       b / nprob of problem b % nprob) at dot_part[b]; their sum is the dot
 *                       product over all blocks.  O is bitwise the same with and without.
 *   CLRSDP_CHAIN_SYM    O_p = L_p (M_p L_p^T) with A1 = M, B1 = A2 = L (the caller passes L as
 *                       both), C1 ignored, a1 scales the inner product.  L MUST be lower
 *                       triangular with exact zeros above its diagonal: the kernel stops the inner
 *                       sums of strip s at k = 32 (s + 1) and skips the row tiles above the strip on
 *                       the strength of those zeros, and it does not check them.  The strip's lower
 *                       part and its mirror image are written: O is exactly symmetric.  halves = 2:
 *                       two pointer sets in one launch (L_X^-1 dX L_X^-T and L_Y^-1 dY L_Y^-T of
 *                       the step length): every array holds 2 nprob blocks, and the second nprob of
 *                       them are given to the kernel as a device allocation of their own.
 *   CLRSDP_CHAIN_TRACE  rout[p][t] = c_agg lam[p][t] ((A1_p B1_p)[:, t] . B1_p[:, t]) + c_in din[p][t]
 *                       for t < ncols: A1_p is n x n (Z), B1_p is n x ncols (V, leading dimension n,
 *                       problem p at offset p n ncols), lam, din, rout hold ncols numbers per
 *                       problem; din may be NULL.  1 <= ncols <= 4096.  A2, O are not used.
 * O (and rout, dot_part) are copied to the device before the launch and back after it.
 * Refused with CLRSDP_E_ARG before any device work: n outside 1 .. 128, nprob outside 1 .. 4096,
 * halves other than 1 (2: CHAIN_SYM only), an unknown form, ncols out of range, a NULL required
 * buffer. */
#define CLRSDP_CHAIN 0
#define CLRSDP_CHAIN_SYM 1
#define CLRSDP_CHAIN_TRACE 2
int32_t clrsdp_gemm_chain(int32_t device, int32_t form, int64_t n, int64_t nprob, int32_t halves,
                          int64_t ncols, double a1, double b1, const double* A1, const double* B1,
                          const double* C1, const double* A2, double* O, const double* DA,
                          const double* DdA, const double* DB, double* dot_part, const double* lam,
                          const double* din, double c_agg, double c_in, double* rout);

/* The reductions that steer the loop (mu = <X,Y>/dim, <c,x>, <b,y>, <C,Y>, max |P|, max |p|,
 * max |d|, min_b lambda_b), each through the launch the solver's stages use: same grid, block
 * and op mapping.  Numbers are `words` planes (1, 2 or 4; hi limb first); the call runs on a
 * stream of its own.  `op` is one of CLRSDP_OP_*; a (kind, op) pair that the solver never issues
 * is CLRSDP_E_ARG.  Every max, min and max-abs is NaN as soon as the leading limb of any element
 * it covers is NaN, at whatever position.
 *   CLRSDP_RED_FLAT_FOLD  flat_reduce over a (b, da, db) of n numbers into CLRSDP_RED_G partials,
 *                         then the fold of the partials inside a scalar_kernel launch (the
 *                         solver's blk_dot at one rank).  DOT, DOTSUM, MAXABS.
 *   CLRSDP_RED_FLAT_TREE  flat_reduce, then vec_reduce over the partials (local_blk_reduce:
 *                         <C,Y>, max |P|, the sharded path).  DOT, DOTSUM, MAXABS.
 *   CLRSDP_RED_VEC        vec_reduce in one workgroup (<c,x>, <b,y>, max |d|).  DOT, MAXABS.
 *   CLRSDP_RED_FOLD       nfold (1 .. 12) folds over the arena a of n numbers, fold q over cnt
 *                         values at a[off + i stride], queued and launched as the solver's
 *                         pending folds are: scalar_kernel launches of at most six folds each
 *                         (fp64: fold_all_f64; multi-word: fold_wave).  The call's op and stride
 *                         are ignored.  out receives nfold numbers.  SUM, MAX, MIN, MAXABS.
 *   CLRSDP_RED_ORDERED    ordered_reduce of n values at a[i stride] (a holds (n - 1) stride + 1
 *                         numbers).  MIN.
 * The FLAT kinds and VEC need stride = 1; b is read by DOT and DOTSUM, da and db by DOTSUM.
 * out: one number (FOLD: nfold).  part (may be NULL; FLAT kinds only): CLRSDP_RED_G numbers, the
 * flat_reduce partials.  out and part are copied to the device before the launch and back after.
 * Refused with CLRSDP_E_ARG before any device work: words, kind or op unknown or not paired, a
 * NULL a or out or required operand, n outside 1 .. 2^28, a stride other than 1 where none is
 * taken, folds with another kind, nfold outside 1 .. 12, a fold that leaves the arena, part with a
 * kind that has no partials. */
#define CLRSDP_RED_FLAT_FOLD 0
#define CLRSDP_RED_FLAT_TREE 1
#define CLRSDP_RED_VEC 2
#define CLRSDP_RED_FOLD 3
#define CLRSDP_RED_ORDERED 4
#define CLRSDP_OP_DOT 0     /* sum a b               */
#define CLRSDP_OP_DOTSUM 1  /* sum (a + da) (b + db) */
#define CLRSDP_OP_SUM 2
#define CLRSDP_OP_MAX 3
#define CLRSDP_OP_MIN 4
#define CLRSDP_OP_MAXABS 5
#define CLRSDP_RED_G 256    /* workgroups, and partials, of flat_reduce and update_state */
typedef struct {
  int64_t cnt, stride, off;
  int32_t op, reserved;
} clrsdp_fold;
int32_t clrsdp_reduce(int32_t device, int32_t words, int32_t kind, int32_t op, int64_t n,
                      int64_t stride, const double* a, const double* b, const double* da,
                      const double* db, int64_t nfold, const clrsdp_fold* folds, double* out,
                      double* part);

/* out[offout + e] = sum_{i < cnt} in[i stride + e] for e < n, in slab_sum4's fixed order (the
 * slabs in four contiguous chunks, eight loads in flight inside each, ((c0 + c1) + (c2 + c3)));
 * with base (n numbers) cbase base[e] + csum sum (without it cbase and csum are not used), and
 * the same numbers to out2 when it is given: Q = sum_j slab_j, p = b - sum_j B_j^T x_j,
 * r = p - sum_j W_j^T t_j.  in holds cnt stride numbers (stride >= n; what lies between n and
 * stride is never read); out and out2 hold nout numbers, are copied to the device before the
 * launch and back after it, and the kernel writes offout .. offout + n only.
 * With Q != NULL (fp64 only, 1 <= n <= 128, out2 NULL) the launch is slab_qsolve: the same r,
 * then out = Q r with the column-major n x n matrix Q of leading dimension ldq (the explicit
 * Q^-1 of the block solve); rows n .. ldq of Q are never read.
 * Refused with CLRSDP_E_ARG before any device work: words other than 1, 2, 4; a NULL in or out;
 * cnt outside 1 .. 65536; n < 1; stride < n; cnt stride > 2^28; a result outside out; with Q:
 * words != 1, n > 128, ldq < n, an out2. */
int32_t clrsdp_slab_sum(int32_t device, int32_t words, int64_t cnt, int64_t stride, int64_t n,
                        const double* in, const double* base, double cbase, double csum,
                        const double* Q, int64_t ldq, double* out, double* out2, int64_t nout,
                        int64_t offout);

/* One update_state launch (the UPDATE stage): X += alpha_p dX, Y += alpha_d dY over nel
 * elements, x += alpha_p dx over nx (0 allowed: x, dx, c may be NULL), y += alpha_d dy over ny,
 * all skipped when one of the ninfo status words info[] is nonzero.  part receives
 * 3 CLRSDP_RED_G numbers: per workgroup the partial <X,Y> of the state the launch leaves
 * (bitwise flat_reduce's partials of it), then those of <c,x> and of <b,y>.
 *   nblk = 0  the slot path: alpha_p and alpha_d are `words` limbs each; eigX, eigY, gamma and
 *             step must be NULL.
 *   nblk > 0  the fused path of a loop body: eigX and eigY hold nblk eigenvalues, gamma `words`
 *             limbs, pd_feas 0 or 1; every workgroup forms the two minima and
 *             alpha = min(1, -gamma / min) (equalised with pd_feas); alpha_p and alpha_d must be
 *             NULL.  step receives four numbers as workgroup 0 writes them: the minimum of
 *             eigX, of eigY, alpha_p, alpha_d.
 * Refused with CLRSDP_E_ARG before any device work: words other than 1, 2, 4; nel < 1, nx < 0,
 * ny < 1, ninfo < 1, nblk < 0; a NULL required buffer; arguments of the other path; pd_feas
 * other than 0 or 1 on the fused path. */
int32_t clrsdp_update_state(int32_t device, int32_t words, int64_t nel, double* X, const double* dX,
                            double* Y, const double* dY, int64_t nx, double* x, const double* dx,
                            const double* c, int64_t ny, double* y, const double* dy,
                            const double* b, int64_t ninfo, const int32_t* info,
                            const double* alpha_p, const double* alpha_d, int64_t nblk,
                            const double* eigX, const double* eigY, const double* gamma,
                            int32_t pd_feas, double* part, double* step);

/* The low-rank operators and block kernels of a handle on operands the caller gives: the
 * operands are copied into the handle's own work buffers as raw limbs (planes of the LOCAL
 * layout of clrsdp_get_buffer: nblk numbers for blocks, nx for tuples; bit copies), the solver's
 * own methods run with the descriptors and plans that build_plans made for this handle, and the
 * result is copied back.  No factorisation and no positive-definite state is needed.  An output
 * buffer is copied to the device first, so what the launches do not write comes back unchanged.
 * Afterwards the handle's work buffers (residuals, directions, scratch) are unspecified: call
 * clrsdp_set_state again before a loop body.  *route tells which kernels ran.
 *   CLRSDP_APPLY_RHS       blocks = Z (taken as given: not symmetrised), tuples = d ->
 *                          tuples_out = -d - Tr(A_* Z): the U = Z V product and direction_rhs_.
 *                          route 0: the strip chain's TRACE form; 1: colsum_rhs;
 *                          2: colsum_dot + tuple_aggregate.
 *   CLRSDP_APPLY_WEIGHTED  tuples = a, blocks = the base -> blocks_out = base + sum_i a_i A_i as
 *                          weighted_A(dx, p_wA_dX, dX, 1.0) forms dX = P + sum_i dx_i A_i (blocks
 *                          with m > 1: of the base's upper block triangle, mirrored).
 *                          route 0: the fused scaled GEMM; 1: scale_cols + GEMM (+ the mirror).
 *   CLRSDP_APPLY_SYM       blocks -> blocks_out = sym(.) with mode 0 ((Z + Z^T)/2), 1 (the upper
 *                          triangle mirrored), 2 (Z^T); only_m != 0: the blocks with m > 1 only.
 *                          Modes 0 and 1 run in place, mode 2 out of place.
 *                          route 0: blk_sym_tiles; 1: blk_sym2.
 *   CLRSDP_APPLY_LIN       mode CLRSDP_LIN_COPY: blocks_out = blocks; CLRSDP_LIN_SUB: blocks_out =
 *                          blocks - blocks2, in place as P - C; CLRSDP_LIN_DIAG: blocks_out =
 *                          blocks + (*scalar) mult I with scalar (`words` limbs) read from a
 *                          device word (diag_add alone).  route 0.
 * CLRSDP_E_ARG: a NULL handle, operand struct, route or required buffer, an unknown op or mode.
 * CLRSDP_E_STATE: constraints not uploaded, or loop bodies in flight. */
#define CLRSDP_APPLY_RHS 0
#define CLRSDP_APPLY_WEIGHTED 1
#define CLRSDP_APPLY_SYM 2
#define CLRSDP_APPLY_LIN 3
#define CLRSDP_LIN_COPY 0
#define CLRSDP_LIN_SUB 1
#define CLRSDP_LIN_DIAG 2
typedef struct {
  const double* blocks;
  const double* blocks2;
  const double* tuples;
  const double* scalar;
  double mult;
  int32_t mode, only_m;
  double* blocks_out;
  double* tuples_out;
} clrsdp_operands;
int32_t clrsdp_apply_operator(clrsdp_handle* h, int32_t op, const clrsdp_operands* a,
                              int32_t* route);

/* The cluster part of the block solve at fp64 in its two launches, through the helpers the loop
 * body calls under CLRSDP_CL_SOLVE=1: cl_solve_t (t_c = L_c^-1 rhs_c and, per 64-row block, its
 * share of W_c^T t_c into slabs), then cl_solve_dx (dx_c = L_c^-T (t_c + W_c dy)); grid
 * ncl x nrb, nrb = ceil(max D / 64).  Cluster c has D[c] rows: Linv holds its D x D matrix
 * (column-major, pitch D; only the lower triangle is read), W its D x ny matrix, rhs, t and dx its
 * D numbers, all concatenated in cluster order; dy holds ny numbers; slabs ncl nrb ny numbers
 * (slab (c nrb + block), zeros for a block past D[c]).  t, slabs and dx are copied to the device
 * before the launches and back after them.
 * Refused with CLRSDP_E_ARG before any device work: a NULL buffer; ncl outside 1 .. 4096; a D
 * outside 1 .. 256; ny < 1; ceil(ny / 64) ncl nrb ny > 2^20 or (ny + 256) doubles beyond 64 KiB
 * (the bounds of the slab_qsolve that sums the slabs). */
int32_t clrsdp_cl_solve(int32_t device, int64_t ncl, const int64_t* D, int64_t ny,
                        const double* Linv, const double* W, const double* rhs, const double* dy,
                        double* t, double* slabs, double* dx);

#ifdef __cplusplus
}
#endif
#endif /* CLRSDP_H */
