/*
 * tunempc_hip.h -- C ABI of the MI355X (gfx950) convexifier.
 *
 * Drop-in boundary for the hot path of TuneMPC, `tunempc/convexifier.py` in the reference:
 * the per-problem SDP that turns the p indefinite stage Hessians H_k of a solved periodic OCP into
 * positive-definite tracking-cost matrices  Hc_k = H_k + dHc_k.  The reference has no native boundary
 * (everything is Python calling PICOS -> CVXOPT/MOSEK); the entry points below are what a ctypes
 * binding of that path binds instead:
 *
 *   reference interface                                    replaced by
 *   ------------------------------------------------------------------------------------------------
 *   convexifier.convexify(A,B,Q,R,N,G,C,opts)               tmpc_convexify_batch_host / _device
 *       (convexifier.py:36-163; Step 1: :98-114)              (B independent problems per call)
 *   convexifier.autoScaling            (:374-401)           inside (k_init_*), reported via info[]
 *   convexifier.setUpModelPicos+solveSDP (:213-308,:359-372) inside (structured primal-dual IPM)
 *   convexifier.check_convergence      (:403-456)           status[] (0 Optimal,1 Feasible,2 Infeasible)
 *   convexifier.convexHessianSuppl     (:165-211)           tmpc_supplement_batch_* and dHc output
 *   opts = {'rho','solver','force'}    (:36)                tmpc_set_options (tol, iteration caps)
 *   Tuner.convexify                    (tuner.py:134-160)   Python side: tunempc_amd.tuner
 *   Pmpc tracking reference W, yref    (pmpc.py:594-609,961-974) tmpc_tracking_reference_host (consumer of Hc, q)
 *   Pocp.get_sensitivities post-processing (pocp.py:322-361) tmpc_pack_sensitivities_host (producer of H, C_As, q)
 *
 * Conventions: plain pointers + sizes, fp64, C (row-major) contiguous arrays:
 *   A  [B][p][nx][nx]      B  [B][p][nx][mb]      H  [B][p][n][n]   (n = nx + mb, H = [[Q,N],[N',R]])
 *   Hc, dHc [B][p][n][n]   P  [B][p][nx][nx]  (P = the reference's un-scaled dP_k, convexifier.py:406)
 * The caller owns every buffer; the library never frees or keeps caller memory.  `_device` variants
 * take device pointers and enqueue on `stream` (a hipStream_t passed as void*); they synchronise the
 * stream internally once per interior-point iteration (a 4-byte "problems still active" read-back).
 * nb = 0 is a no-op that returns TMPC_OK (an empty shard of a batch split over several GPUs).
 * Unit-test and diagnostic entry points are declared in tunempc_hip_debug.h, not here.
 * All functions return 0 on success or a negative TMPC_E_* code; per-problem solver outcomes are in
 * status[] so that one infeasible member does not abort a batch.
 */
#ifndef TUNEMPC_HIP_H
#define TUNEMPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMPC_OK 0
#define TMPC_E_ARG (-1)        /* bad argument (null pointer, non-positive size)            */
#define TMPC_E_UNSUPPORTED (-2) /* shape outside what the handle / entry supports: nx+mb > 96 (> 64 with rows or Step 3), more than TMPC_MAX_ROWS rows, Schur blocks wider than 3168, p < 1; tight mode on a handle with rows */
#define TMPC_E_NOMEM (-3)      /* hipMalloc failed                                          */
#define TMPC_E_HIP (-4)        /* HIP runtime error (see tmpc_last_error)                   */
#define TMPC_E_NODEVICE (-5)   /* no gfx950 device visible                                  */
#define TMPC_E_NOCONV (-6)     /* tmpc_eig_clip_host: Jacobi sweeps exhausted (outputs hold the last iterate) */

#define TMPC_STATUS_OPTIMAL 0    /* convexifier.py:444 'Optimal'    */
#define TMPC_STATUS_FEASIBLE 1   /* convexifier.py:446 'Feasible'   */
#define TMPC_STATUS_INFEASIBLE 2 /* convexifier.py:451 'Infeasible' */

#define TMPC_FLAG_NO_MFMA 1      /* debug: scalar-FMA GEMM fragments on the register-staged kernels instead of the matrix cores (product path: v_mfma_f64_4x4x4 tiles fed by LDS-DMA) */
#define TMPC_FLAG_PROFILE 2      /* record hipEvent timings per phase (tmpc_get_profile)           */
#define TMPC_FLAG_FAST_EXIT 4    /* stop every problem after its FIRST full centering step instead of converging to the central-path point
                                    at mu_target: Hc is feasible (positive definite, cond <= kappa), kappa within the same gap N mu_target of
                                    optimal, the linear residuals are gone -- but the point is within ~1e-2 (relative) of the centred one, not
                                    at it, so two implementations agree on it to ~1e-3 only, not to 1e-8.  ~2 factorisations fewer per problem.
                                    Members stopped this way carry info[10] = 3.  Off by default: the default answer is the reproducible one. */

#define TMPC_INFO_STRIDE 16      /* doubles per problem in info[] (layout below)                   */
/* info[b*16 + i]: 0 s (=1/min|eig H|), 1 sbeta, 2 min eig H, 3 min eig Hc, 4 max cond Hc, 5 mu,
 *                 6 mu_target, 7 pinf, 8 dinf, 9 relgap, 10 ipm status (0 opt,1 inaccurate,2 maxiter,3 = stopped by TMPC_FLAG_FAST_EXIT: status Optimal, not the converged point,
 *                    4 = tight mode only: the continuation of this member failed and the result of its DEFAULT solve was returned -- status Optimal at the default gap, info[6]),
 *                 11 #shifted pivots, 12 centering iterations, 13 early-exit flag (convexifier.py:83-85),
 *                 14 last centering step norm, 15 smallest Cholesky pivot of the Schur factorisations relative to the assembled diagonal (1 if never below 1e-8; <= 1e-15 = frozen)                                          */

typedef struct tmpc_handle tmpc_handle;

/* Number of HIP devices visible (0 if none / HIP not initialisable).  Never touches a device. */
int tmpc_device_count(void);

/* Device workspace needed for `chunk` problems of shape (p, nx, mb), in bytes (0 if unsupported).
 * Supported: p >= 1, nx + mb <= 64 for every model (tuned per-stage kernels up to 32, generic ones above) and <= 96 for the plain model (no G / C rows, no Step 3),
 * rows of G_k / C_k up to TMPC_MAX_ROWS each, and
 * Schur blocks -- nx(nx+1)/2, plus the rows, plus (Step 3) the (nx+mb)(nx+mb+1)/2 + 1 entries of T_k and its epigraph variable -- of at most 3168 (round 4: 2384). */
uint64_t tmpc_workspace_bytes(int chunk, int p, int nx, int mb);

/* Create a handle on the current HIP device with workspace for `chunk` problems per launch wave.
 * Larger batches are processed in chunks.  chunk <= 0 selects a default that fits free HBM. */
int tmpc_create(tmpc_handle** out, int chunk, int p, int nx, int mb);
#define TMPC_MAX_ROWS 31         /* rows of G_k, and rows of C_k, per stage (each)                     */
#define TMPC_ARROW_LD 32         /* leading dimension of the arrow blocks tmpc_get_dual_con_host exports */
/* The same with room for `ng` equality-constraint rows per stage (0 <= ng <= TMPC_MAX_ROWS), for tmpc_convexify_eq_batch_host.
 * Such a handle also serves every call that takes no G. */
uint64_t tmpc_workspace_bytes_eq(int chunk, int p, int nx, int mb, int ng);
int tmpc_create_eq(tmpc_handle** out, int chunk, int p, int nx, int mb, int ng);
/* The same with room for up to `nc` active-constraint rows per stage as well (0 <= nc <= TMPC_MAX_ROWS),
 * for tmpc_convexify_step2_batch_host. */
uint64_t tmpc_workspace_bytes_con(int chunk, int p, int nx, int mb, int ng, int nc);
int tmpc_create_con(tmpc_handle** out, int chunk, int p, int nx, int mb, int ng, int nc);
int tmpc_destroy(tmpc_handle* h);
/* Problems processed per launch wave (the chunk the workspace was sized for). */
int tmpc_get_chunk(tmpc_handle* h);

/* Solver options: tol = complementarity tolerance mu_target/kappa per unit cone dimension, default 2^-25
 * (the relative duality gap on kappa, the max condition number, is then (2*p*n+1)*tol);
 * center_tol = relative Newton step ending the final centering phase, default 1e-9;
 * max_iter / center_iter = iteration caps (defaults 50 / 12): max_iter bounds the main phase, center_iter the centering iterations
 * per barrier target (a chord step, which re-uses the factorisation at a fifth of the cost, counts a quarter: up to 4 x center_iter cheap iterations) -- a hard target may visit up to 11 targets (ten back-offs by powers of two, reported in info[6]), so a problem ends
 * after at most max_iter + 11 * center_iter + 2 iterations; flags = TMPC_FLAG_*.  Values <= 0 keep
 * the current setting (flags is always applied; bits other than the TMPC_FLAG_* above -- and the debug bit of
 * tunempc_hip_debug.h -- are rejected with TMPC_E_ARG). */
int tmpc_set_options(tmpc_handle* h, double tol, double center_tol, int max_iter, int center_iter, int flags);

/* Performance knobs of a handle (none of them changes WHAT is computed beyond rounding; defaults are the measured optimum on MI355X):
 *   TMPC_TUNE_CHORD_STEP   value > 0: the centering phase re-uses a factorisation once a full Newton step could have been `value` times longer
 *                          before leaving the cone (default 10); 0: every centering step re-factors
 *   TMPC_TUNE_SMALL_BLOCKS 1 (default): blocks of one 16 x 16 tile (the reference's own examples, nx <= 5) are factored / solved by ONE kernel per
 *                          problem; 0: the batched launch sequence per elimination level
 *   TMPC_TUNE_EIG_PRETEST  1 (default): the step-length kernel first asks whether the step at the clipping threshold stays in the cone; 0: every
 *                          eigenvalue is computed
 *   TMPC_TUNE_FUSE_FWD     1 (default): the forward substitution of the predictor pass rides inside the factorisation; 0: separate sweep
 *   TMPC_TUNE_GRAPH        1 (default): problems whose Schur blocks are a single tile (nx <= 10: launch-bound) replay the launch sequence of an iteration as a
 *                          captured hipGraph (one submission instead of ~35; the handle's own streams only); 0: plain launches
 *   TMPC_TUNE_LOWP_SWITCH  value >= 0 (default TMPC_LOWP_SWITCH_DEFAULT): in the main-phase iterations of a problem with mu > value * max(1, |tau|) (tau: the
 *                          current objective estimate, kappa at the end; the value is raised to 16 tol if below it) the Schur-complement updates of
 *                          the block factorisation (k_cr_update_dma, a third of a solve) run on float32 copies of their operands with float32 accumulation (fp32 MFMA:
 *                          twice the fp64 matrix rate); the Cholesky of the diagonal blocks and every later iteration stay fp64 (the triangular solves: TMPC_TUNE_LOWP_TRSM).  Same iteration counts, the
 *                          converged point moves by 1e-11 ... 2e-10 (profiles/r6_fp32_*.txt).  Steps 1 and 2 (not Step 3), stage blocks up to 32 x 32, Schur blocks of 80 ... 320; a pivot that freezes under
 *                          them repeats the iteration in fp64 and turns them off for that problem.  0: never (rounds 1-5, bit for bit)
 *   TMPC_TUNE_LOWP_TRSM    1 (default): in those same iterations the triangular solves O = E L^-T of the factorisation run in single precision as well
 *                          (k_cr_trsm_dma_f32: fp64 operands rounded on the fragment read, float32 accumulation, only the float32 copy of O is produced -- the one
 *                          the updates and substitutions of such an iteration read); the Cholesky of the diagonal blocks stays fp64.  0: fp64 solves in every
 *                          iteration (round 6, bit for bit)
 *   TMPC_TUNE_TRSM_PAIR    1 (default): a workgroup of k_cr_trsm_dma_f32 solves strip r of BOTH edge blocks of an eliminated node on one stream of the node's
 *                          factor (one item per problem, node and strip; each L fragment read and rounded once for the two edges); 0: one edge per workgroup
 *                          (round 7's item list).  Same MFMA sequence per output element: bit-identical results
 *   TMPC_TUNE_PERSISTENT   plain-model problems with single-tile Schur blocks and n = nx + mb <= 8 (the reference's own examples) can run their whole
 *                          interior-point loop as ONE launch, one workgroup per problem (tmpc_persist.h).  1 (default): where that is faster -- period
 *                          p <= 8, or at least 96 problems of the call on the chip at once; 0: never (the launch sequence); 2: whenever the shape allows it
 * (Rounds 1-3 read these from environment variables once per process.) */
#define TMPC_TUNE_CHORD_STEP 1
#define TMPC_TUNE_SMALL_BLOCKS 2
#define TMPC_TUNE_EIG_PRETEST 3
#define TMPC_TUNE_FUSE_FWD 4
#define TMPC_TUNE_GRAPH 5
/* (key 6 belonged to two measured-and-dropped experiments -- rounds 5 and 6, profiles/r5_fused_elim.txt, profiles/r6_update_stream_*.txt -- and is not reused) */
#define TMPC_TUNE_PERSISTENT 7
#define TMPC_TUNE_LOWP_SWITCH 8
#define TMPC_LOWP_SWITCH_DEFAULT 1e-5
#define TMPC_TUNE_LOWP_TRSM 9
#define TMPC_TUNE_TRSM_PAIR 10
int tmpc_set_tuning(tmpc_handle* h, int key, double value);
/* The general constructor: ng / nc rows of G_k / C_k (0: none), step3 != 0: room for T_k, lanes = concurrent half-waves on their own streams
 * (0: automatic -- two for problems whose blocks are a single 64 x 64 tile and chunk >= 2, one otherwise; at most 4). */
int tmpc_create_ex(tmpc_handle** out, int chunk, int p, int nx, int mb, int ng, int nc, int step3, int lanes);

/* Tight-accuracy mode (opt-in; Step 1 and Step 2 handles with nx <= 51 and nx + mb <= 64; with rows of G / C -- round 5 -- while
 * rows * (2 (nx + mb) + 2 nx) <= 4040; no Step 3).  The reference hands its SDP to MOSEK / CVXOPT, which stop at a relative gap of
 * ~1e-8 (convexifier.py:363); the default solve above stops at tol = 2^-25, a certified gap of (2*p*n+1)*3e-8 on kappa, because the HKM
 * Schur matrix (condition ~1/mu^2) cannot be factored in fp64 below mu ~ 1e-8.  With enable != 0 every problem that ended Optimal is
 * continued from its centred point towards mu_target = tight_tol * kappa (default 2^-37 ~ 7.3e-12: gap (2*p*n+1)*7.3e-12; accepted range
 * [2^-42, 1), every member of the test families converges down to 2^-37, most down to 2^-41) with the Kronecker-factor images, the
 * assembly, the block Cholesky and the substitutions in double-double arithmetic, and finished by Newton steps on the dual barrier
 * problem in which every stage quantity is double-double (the returned point is then reproducible to ~1e-12 instead of ~eps/mu).
 * Outputs as before; info[6] = the mu_target reached, iters includes the extra iterations.  A member whose continuation fails (a non-positive
 * double-double pivot, a polish step that leaves the cone, the iteration cap: most visibly hard targets below 2^-33) gets the result of its default
 * solve back, status Optimal, info[10] = 4 and info[6] = the default's mu_target: the mode never returns less than the default does, and says so.  Costs one more workspace of about the size of
 * the block storage (allocated at the first enable) and ~10 double-double factorisations per problem (vector ALU, no matrix cores).
 * With rows (Step 1 with G; the Step 2 model with either objective) the multipliers and the epigraph variables of the norm terms ride in the augmented blocks
 * as in the default solve, their rows formed in double-double, and join the polish as variables; tmpc_get_dual_host / tmpc_get_dual_con_host export the dual
 * iterate that goes with the last Newton step of the polish (LMI blocks, multipliers z, primal blocks of the norm terms): it certifies the gap to ~N * tight_tol.
 * enable == 0 switches back to the default (the workspace stays).  TMPC_E_UNSUPPORTED for Step 3 handles and for rows beyond the limits above. */
int tmpc_set_tight(tmpc_handle* h, int enable, double tight_tol);

/* Step 1 of convexifier.convexify for `nb` independent problems.  Any output pointer may be NULL.
 * status/iters are int32 [nb]; alpha/beta/kappa are double [nb]; info is double [nb][16]. */
int tmpc_convexify_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* H,
                              double* Hc, double* dHc, double* P, double* alpha, double* beta, double* kappa,
                              int32_t* status, int32_t* iters, double* info);
int tmpc_convexify_batch_device(tmpc_handle* h, int nb, const double* dA, const double* dB, const double* dH,
                                double* dHc_out, double* ddHc_out, double* dP_out, double* d_alpha, double* d_beta,
                                double* d_kappa, int32_t* d_status, int32_t* d_iters, double* d_info, void* stream);

/* Step 1 with the equality-constraint term (convexifier.py:249-255 multipliers Fg_k >= 0, :346-347 term G_k' diag(Fg_k) G_k
 * in M_k, :409-411 un-scaling): G [nb][p][ng][n] with ng of tmpc_create_eq; Fg [nb][p][ng] out.  dHc includes the G term
 * (convexifier.py:196-197).  The multipliers of stage k ride inside block k+1 of the block factorisation
 * (tunempc_amd/csrc/tmpc_phi.h). */
int tmpc_convexify_eq_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* H, const double* G,
                                 double* Hc, double* dHc, double* P, double* Fg, double* alpha, double* beta, double* kappa,
                                 int32_t* status, int32_t* iters, double* info);

/* The model of Step 2 (convexifier.py:116-131: setUpModelPicos with constr=True, :258-266 multipliers F_k >= 0 of the active
 * constraints, :276-283 objective beta + sum rho*||F_k|| + sum rho*||Fg_k||, :348-350 term C_k' diag(F_k) C_k, :415-420 un-scaling).
 * J [nb][p][ng+nc][n]: per stage the ng rows of G_k, then the rows of C_k, zero padding up to nc (ng, nc of tmpc_create_con);
 * ncnt int32 [nb][p]: rows of C_k actually present (0 for a stage whose C_k is None).  FgF [nb][p][ng+nc] out: Fg_k, then F_k,
 * zeros in the padding.  dHc includes both constraint terms.  The caller decides when to take this step (after Step 1 came
 * back Infeasible, as convexify() does).
 * rho = 0 selects the BETA-ONLY objective: the reference assembles the norm terms with `picos.sum(obj, abs(rho*F[i]))`
 * (convexifier.py:276-283); whether PICOS 1.2.0 adds or drops that second argument cannot be checked here (the package is not installed,
 * SURVEY.md 7.0).  If it drops it, the solver sees min beta with cost-free multipliers F_k, Fg_k >= 0 -- the rows of C_k then act exactly
 * like rows of G_k -- which is what rho = 0 solves (no norm cones at all, not a zero-weight limit of them).  rho > 0 is the paper's
 * objective (eq. 20a) and the default of the Python mirror. */
int tmpc_convexify_step2_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* H, const double* J,
                                    const int32_t* ncnt, double rho, double* Hc, double* dHc, double* P, double* FgF, double* alpha,
                                    double* beta, double* kappa, int32_t* status, int32_t* iters, double* info);

/* The model of Step 3 (convexifier.py:137-147: setUpModelPicos with force=True, :269-273 T_k symmetric with every entry > 0, :284-285
 * objective + sum rho*||T_k||_F, :352-353 term s_T*T_k, :422-423 un-scaling), here for the plain model (no G / C rows in the same solve):
 * handle from tmpc_create_step3; T [nb][p][n][n] out; dHc includes T_k (convexifier.py:202-203).  The caller decides when to take
 * this step (after the earlier steps came back Infeasible and with the 'force' option, as convexify() does).  The norm term is a
 * second-order cone handled natively (tunempc_amd/csrc/tmpc_t3.h); the blocks of the factorisation grow to d + n(n+1)/2 + 1. */
uint64_t tmpc_workspace_bytes_step3(int chunk, int p, int nx, int mb);
int tmpc_create_step3(tmpc_handle** out, int chunk, int p, int nx, int mb);
int tmpc_convexify_step3_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* H, double rho,
                                    double* Hc, double* dHc, double* P, double* T, double* alpha, double* beta, double* kappa,
                                    int32_t* status, int32_t* iters, double* info);

/* Step 3 with the multipliers of G and C in the same solve (convexifier.py:144: setUpModelPicos(..., constr = constraint_contribution,
 * force = True)): handle from tmpc_create_step3_con (ng, nc as in tmpc_create_con); J, ncnt, FgF as in tmpc_convexify_step2_batch_host;
 * ncnt == NULL: no C rows -- J holds the ng rows of G only, cost-free multipliers as in tmpc_convexify_eq_batch_host (the reference's
 * constr = False).  T [nb][p][n][n] out; dHc includes the constraint terms and T_k. */
uint64_t tmpc_workspace_bytes_step3_con(int chunk, int p, int nx, int mb, int ng, int nc);
int tmpc_create_step3_con(tmpc_handle** out, int chunk, int p, int nx, int mb, int ng, int nc);
int tmpc_convexify_step3_con_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* H, const double* J,
                                        const int32_t* ncnt, double rho, double* Hc, double* dHc, double* P, double* FgF, double* T,
                                        double* alpha, double* beta, double* kappa, int32_t* status, int32_t* iters, double* info);
/* Device-resident forms of the two Step 3 entries (device pointers in and out; `stream`: the caller's HIP stream, NULL = default -- the call returns
 * with every result written, as tmpc_convexify_batch_device). */
int tmpc_convexify_step3_batch_device(tmpc_handle* h, int nb, const double* dA, const double* dB, const double* dH, double rho, double* Hc, double* dHc,
                                      double* P, double* T, double* alpha, double* beta, double* kappa, int32_t* status, int32_t* iters, double* info, void* stream);
int tmpc_convexify_step3_con_batch_device(tmpc_handle* h, int nb, const double* dA, const double* dB, const double* dH, const double* dJ, const int32_t* d_ncnt,
                                          double rho, double* Hc, double* dHc, double* P, double* FgF, double* T, double* alpha, double* beta, double* kappa,
                                          int32_t* status, int32_t* iters, double* info, void* stream);

/* Device-resident form of the two entries above (inputs and outputs in HBM, work queued on `stream`): d_ncnt == NULL is Step 1
 * with G (dJ = G [nb][p][ng][n], FgF [nb][p][ng]); otherwise the Step 2 model (dJ [nb][p][ng+nc][n], d_ncnt [nb][p] with
 * 0 <= ncnt <= nc -- not checked here --, FgF [nb][p][ng+nc]). */
int tmpc_convexify_con_batch_device(tmpc_handle* h, int nb, const double* dA, const double* dB, const double* dH, const double* dJ,
                                    const int32_t* d_ncnt, double rho, double* dHc_out, double* ddHc_out, double* dP_out, double* dFgF,
                                    double* d_alpha, double* d_beta, double* d_kappa, int32_t* d_status, int32_t* d_iters,
                                    double* d_info, void* stream);

/* convexHessianSuppl (convexifier.py:165-211) alone: dHc_k = sym(V_k' P_{k+1} V_k - E' P_k E). */
int tmpc_supplement_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* P, double* dHc);
/* The same with the constraint and regularisation terms of convexifier.py:196-204:
 *   dHc_k = sym(V_k' P_{k+1} V_k - E' P_k E + J_k' diag(w_k) J_k + T_k),
 * J [nb][p][nr][n]: rows of G_k (weights Fg_k) followed by rows of C_k (weights F_k), zero-weight padding up to nr rows
 * per stage (ragged C_k, per-stage None = all weights zero); wts [nb][p][nr]; T [nb][p][n][n].  J/wts and T may be NULL. */
int tmpc_supplement_terms_batch_host(tmpc_handle* h, int nb, const double* A, const double* B, const double* P, int nr,
                                     const double* J, const double* wts, const double* T, double* dHc);

/* Producer side: the array post-processing of Pocp.get_sensitivities (pocp.py:322-361) that turns the raw NLP sensitivities into
 * the inputs of convexify(), for nb problems at once (p, n = nx + mb of the handle):
 *   C [nb][p][nh][n] path-constraint Jacobians and mu [nb][p][nh] their multipliers (both NULL: no path constraints):
 *     C_As [nb][p][ncmax][n] = the rows with |mu| > thr in their original order, zero-padded (pocp.py:322-340; threshold :73),
 *     ncnt [nb][p] their number (a value > ncmax means the padding was too small), idx [nb][p][nh] their row indices (-1 padding,
 *     may be NULL), q [nb][p][n] = -mu' C (pocp.py:357-361; zeros without constraints; may be NULL);
 *   Hbig [nb][p*n][p*n] Lagrangian Hessian of the whole NLP (may be NULL): Hst [nb][p][n][n] its diagonal stage blocks (:350-355).
 * C_As / ncnt are the J / ncnt inputs of tmpc_convexify_step2_batch_host. */
int tmpc_pack_sensitivities_host(tmpc_handle* h, int nb, int nh, const double* C, const double* mu, const double* Hbig, double thr, int ncmax,
                                 double* C_As, int32_t* ncnt, int32_t* idx, double* q, double* Hst);

/* Consumer side of the tuned matrices, the tracking-MPC reference update (pmpc.py:961-974; set-up :594-609):
 *   W_k = sym(Hc_k) / ts,   yref_k = wref_k - (Hc_k/ts)^-1 q_k / ts = wref_k - Hc_k^-1 q_k      for nstage independent stages.
 * Hc [nstage][n][n] (n = nx + mb of the handle), q, wref, yref [nstage][n], W [nstage][n][n]; info[k] = number of
 * non-positive Cholesky pivots of Hc_k (0 for every matrix convexify() reports Optimal/Feasible).  W, info may be NULL. */
int tmpc_tracking_reference_host(tmpc_handle* h, int nstage, const double* Hc, const double* q, const double* wref,
                                 double ts, double* W, double* yref, int32_t* info);

/* Stage-block eigen scan (pre-check convexifier.py:82, autoScaling :374-401, status check :438-440):
 * out[b*p+k][0..3] = min eig, max eig, min |eig| (zeros excluded), max |eig| of sym(H[b][k]). */
int tmpc_eig_scan_host(tmpc_handle* h, int nb, const double* H, double* out);

/* Eigenvalue clip of general-size symmetric matrices (reference: tunempc/sqp_method.py:327-403, `Sqp.__regularize_hessian`: the
 * eigenvalues of the (reduced) Hessian below `regularization_tol` are lifted to it, H += evec diag(evmod - eva) evec^-1):
 *   out[b] = sym(A[b]) + V diag(max(tol - lambda_i, 0)) V',   A, out [nb][n][n], any n >= 1 (no handle, current device).
 * evals [nb][n] (optional): the eigenvalues lambda_i of A[b] (unordered); reg [nb] (optional): the largest lift max_i(tol - lambda_i, 0)
 * (the reference's `self.__reg`); sweeps [nb] (optional): Jacobi sweeps taken.  Returns TMPC_E_NOCONV when 40 sweeps did not
 * orthogonalise the vectors to the rounding level (~2 sqrt(n) eps); the outputs then hold the last iterate. */
int tmpc_eig_clip_host(int nb, int n, const double* A, double tol, double* out, double* evals, double* reg, int32_t* sweeps);

/* Periodic LQR gains: the local feedback law of a (tuned) scheme, its cost-to-go and closed-loop monodromy (reference: convexifier.py:44-45, the LQR
 * problems on H and on Hc = H + dHc share their feedback law; examples/convex_lqr.py:52-58).  Stage k of problem b, indices mod p, x block of H first:
 *     E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,  K_k = S^-1 M  (u = -K_k x, the sign of scipy / control.dare),
 *     Pi_k = sym(Hb_xx - M' K_k).
 * A sweep runs k = p-1 ... 0 starting from Pi = Pi0 [nb][p][nx][nx] (NULL: zero; the sweep reads Pi0_0 first, the other stages only enter the change
 * measure); sweeps repeat until max_k max|Pi_k - Pi_k(previous sweep)| / max(1, max|Pi_k|) <= tol or max_sweeps is reached, all inside one launch.
 * A [nb][p][nx][nx], B [nb][p][nx][mb], H [nb][p][n][n] (n = nx + mb <= TMPC_LQR_NMAX, any p, nb >= 1).  Outputs: K [nb][p][mb][nx], Pi [nb][p][nx][nx],
 * Phi [nb][nx][nx] (optional) = (A_{p-1} - B_{p-1} K_{p-1}) ... (A_0 - B_0 K_0), and per problem info [nb][8]:
 *   [0] status: 0 converged, 1 max_sweeps reached (K, Pi, Phi hold the last iterate), 2 S numerically singular at a stage, 3 non-finite iterate
 *       (2, 3: the problem stops there, Phi is NaN, K / Pi hold what was written until then; other problems are not affected),
 *   [1] sweeps used, [2] last relative change, [3] / [4] smallest / largest |pivot| of S over the last sweep,
 *   [5] 1.0 if the elimination of the last sweep never left a positive diagonal pivot (S positive definite at every stage; 0.0: not shown),
 *   [6] the same over EVERY sweep of the call (at a converged Pi the S of the H side equals the positive definite S of the Hc side, so [5] reads 1 there
 *       whatever the path was; [6] tells whether the path from Pi0 met an indefinite S), [7] reserved.
 * S is solved by elimination with row pivoting, so a symmetric indefinite S (the usual case from Pi0 = 0 with an indefinite H) is handled.
 * With the P of a convexification (Hc_k = H_k + calH_k(P)) the H-recursion from Pi0 = +P is the Hc-recursion from zero shifted by P, iterate by iterate.
 * Returns TMPC_OK when the call ran; TMPC_E_UNSUPPORTED for nx + mb > TMPC_LQR_NMAX (checked before the device is touched).
 * _host: host pointers (device scratch kept between calls).  _device: device pointers, current device, null stream, synchronised before returning. */
#define TMPC_LQR_NMAX 64
int tmpc_periodic_lqr_batch_host(int nb, int p, int nx, int mb, const double* A, const double* B, const double* H, const double* Pi0, double tol,
                                 int max_sweeps, double* K, double* Pi, double* Phi, double* info);
int tmpc_periodic_lqr_batch_device(int nb, int p, int nx, int mb, const double* A, const double* B, const double* H, const double* Pi0, double tol,
                                   int max_sweeps, double* K, double* Pi, double* Phi, double* info);

/* The same recursion for the models with rows: stage k holds J_k [x_k; u_k] = 0 with J_k = [G_k; C_k[:ncnt_k]] = [Jx | Ju] (first nx | last mb columns),
 * r_k = ng + ncnt_k rows -- the J / ncnt layout of tmpc_convexify_step2_batch_host.  Per stage
 *     [ S   Ju' ] [ K_k   ]   [ M  ]
 *     [ Ju  0   ] [ Lam_k ] = [ Jx ]       u = -K_k x,   Pi_k = sym(Hb_xx - [M; Jx]' [K_k; Lam_k]),   Jx - Ju K_k = 0.
 * Hc_k = H_k + calH_k(P) + J_k' diag(phi_k) J_k and the last term vanishes on J_k w = 0: the constrained problems on H (from Pi0 = +P) and on Hc (from zero)
 * have the same K_k and Pi_k(H) = Pi_k(Hc) + P_k iterate by iterate, which the unconstrained ones lose as soon as a multiplier phi is non-zero.
 * Arguments of the plain entries plus: nr row capacity per stage (>= ng), ng rows present at every stage, J [nb][p][nr][n] (rows beyond r_k are not read),
 * ncnt int32 [nb][p] (NULL: ng rows at every stage), Lam [nb][p][nr][nx] (optional; the multiplier gains, zero beyond r_k).
 * Served: r_k <= mb with Ju of full row rank.  info as above, with
 *   [0] status 4: r_k > mb (or r_k > nr, ncnt_k < 0) at some stage, decided before the first sweep ([1] = 0; K, Lam zero, Pi = Pi0, Phi NaN);
 *       status 2 also covers a rank-deficient Ju (in particular rows on the state alone: they need a constraint-to-go recursion, not provided),
 *   [3] / [4] pivots of the whole KKT matrix, [5] / [6] 1.0 if every elimination took mb positive and then r_k negative diagonal pivots (S positive
 *       definite and Ju of full row rank: a convex stage problem), [7] max_k max|Jx - Ju K_k| of the returned gains (0 when status >= 2).
 * With r_k = 0 at every stage the outputs are those of the plain entry, bit for bit.  TMPC_E_ARG: nr < ng, (host entry) ncnt outside 0 .. nr - ng;
 * TMPC_E_UNSUPPORTED (before the device is touched): nx + mb > TMPC_LQR_NMAX, or (nx, mb, nr) beyond 160 KB of LDS -- n <= 32 fits with any nr <= 66,
 * 32 < n <= 64 with any nr <= 15 and with more where the split of n leaves room (nx = mb = nr = 32 fits). */
int tmpc_periodic_lqr_rows_batch_host(int nb, int p, int nx, int mb, int nr, int ng, const double* A, const double* B, const double* H, const double* J,
                                      const int32_t* ncnt, const double* Pi0, double tol, int max_sweeps, double* K, double* Pi, double* Phi, double* Lam,
                                      double* info);
int tmpc_periodic_lqr_rows_batch_device(int nb, int p, int nx, int mb, int nr, int ng, const double* A, const double* B, const double* H, const double* J,
                                        const int32_t* ncnt, const double* Pi0, double tol, int max_sweeps, double* K, double* Pi, double* Phi, double* Lam,
                                        double* info);

/* The recursion with rows for ANY rows: more rows than inputs (r_k > mb), rows on the state alone, dependent rows (tmpc_lqr_ctg.h).  What the rows of stage k
 * and of the stages after it say about x_k alone is carried backwards as a constraint-to-go Hn_k x_k = 0 (c_k orthonormal rows, empty at the start):
 *     Cf = [J_k; Hn_{k+1} [A_k B_k]] is split by elimination with full pivoting on its u columns -- a pivot is accepted while the largest remaining |entry|
 *     exceeds rank_tol * max(1, max|Cf|) -- into rho <= mb rows [Jx~ | Ju~] of full row rank and rows with a zero u part, whose x parts are compressed
 *     (Gram-Schmidt with row pivoting, same threshold) to Hn_k;  [[S, Ju~'], [Ju~, 0]] [K; Lam] = [M; Jx~] as in the rows entry (rho = mb allowed);
 *     Pz = I - Hn_k' Hn_k,  K_k = K Pz,  Pi_k = sym(Pz (Hb_xx - [M; Jx~]' [K; Lam]) Pz)    (unique; off the feasible subspace u = -K_k x says nothing).
 * Sweeps stop when the change measure of the plain entry is <= tol and no c_k changed during the sweep.
 * Arguments of the rows entries plus rank_tol (> 0; 1e-9 is the library's default in Python); no Lam (the multipliers are not unique).  Outputs:
 * K, Pi as before; Phi (optional) = (A-BK)_{p-1} ... (A-BK)_0 Pz_0; Hn [nb][p][nx][nx], rows beyond c_k zero; cnt int32 [nb][p] = c_k; info [nb][12]:
 *   [0] status 0 .. 3 as above (2: singular reduced Hessian of a stage), 5 no feasible subspace (c_k reached nx: only x_k = 0 satisfies the rows; the problem
 *       stops there, Phi NaN); status 4 is never returned, ncnt is clamped to 0 .. nr - ng;
 *   [1] .. [6] as in the rows entry (the rows enter the elimination scaled to the largest diagonal entry of S, so they compete with its diagonal for the pivot
 *       and [5] / [6] read 0, "not shown", more often than in the rows entry), [7] max_k max(|(Jx - Ju K_k) Pz_k|, |Hn_{k+1} (A_k - B_k K_k) Pz_k|) of the returned gains (0 when status >= 2),
 *   [8] sum_k c_k and [9] max_k c_k of the last sweep, [10] smallest accepted and [11] largest rejected pivot of all splits and compressions of the call,
 *       relative to the stage scale max(1, max|Cf|) ([10] = inf, [11] = 0 when there was none): a decision is safe when [11] << rank_tol << [10].
 * TMPC_E_ARG: nr < ng, rank_tol <= 0, NULL Hn / cnt, (host entry) ncnt outside 0 .. nr - ng.  TMPC_E_UNSUPPORTED (before the device is touched):
 * nx + mb > TMPC_LQR_NMAX, or (nx, mb, nr) beyond 160 KB of LDS -- the layout holds the stack twice, [max(nr + nx, mb)][n], and Hn twice. */
#define TMPC_LQR_CTG_INFO 12
int tmpc_periodic_lqr_ctg_batch_host(int nb, int p, int nx, int mb, int nr, int ng, const double* A, const double* B, const double* H, const double* J,
                                     const int32_t* ncnt, const double* Pi0, double tol, double rank_tol, int max_sweeps, double* K, double* Pi, double* Phi,
                                     double* Hn, int32_t* cnt, double* info);
int tmpc_periodic_lqr_ctg_batch_device(int nb, int p, int nx, int mb, int nr, int ng, const double* A, const double* B, const double* H, const double* J,
                                       const int32_t* ncnt, const double* Pi0, double tol, double rank_tol, int max_sweeps, double* K, double* Pi, double* Phi,
                                       double* Hn, int32_t* cnt, double* info);

/* Finite-horizon gains: the first-order feedback u_0 = -K_0 x_0 of the horizon-N problem that starts at phase k0 of the p-periodic model, for a list of
 * starting phases (tmpc_lqr_horizon.h; reference pmpc.py:162-281, the LQ content of closed_loop_tools.check_equivalence).  One backward pass j = N-1 ... 0 over
 * the stages k = (k0 + j) mod p per (problem, phase), no convergence loop; N may be smaller than, equal to or larger than p.  The stage is that of the ctg
 * entry, so any rows are served; the pass starts from Pi_N = Pf[(k0 + N) mod p] (Pf [nb][p][nx][nx]; NULL: zero) and
 *     terminal = 0 (cost):        Hn_N empty;
 *     terminal = 1 (constraint):  Hn_N = I, i.e. x_N = 0 (c_N = nx is legal at this given stage only; a general terminal operator is not provided).
 * Arguments of the ctg entry (nr = 0 with J = NULL allowed) plus N, nph and phases: int32 [nph], a HOST pointer in both entries (NULL: all p phases in order,
 * nph must then equal p).  Outputs per (problem, phase): K0 [nb][nph][mb][nx], Pi0 [nb][nph][nx][nx], Hn0 [nb][nph][nx][nx] (rows beyond c_0 zero), all projected
 * on the feasible subspace of x_0 as in the ctg entry; cnt0 int32 [nb][nph] = c_0; optional Kall [nb][nph][N][mb][nx] and cntall int32 [nb][nph][N], the gains
 * and counts of every stage j of the pass (large: nb nph N mb nx doubles); info [nb][nph][12]:
 *   [0] status: 0 done, 2 singular stage system, 3 non-finite, 5 no feasible subspace (a computed c_j reached nx); 1 and 4 are never returned.  With status >= 2
 *       K0 and Pi0 are NaN, Hn0 is zero, cnt0 is the count at the failing stage (nx for status 5), and the stages of Kall / cntall that were not finished hold
 *       NaN / -1.  One (problem, phase) never affects another;
 *   [1] N, [2] stages finished, [3] / [4] smallest / largest |pivot| of the stage systems, [5] = [6] 1.0 if every stage problem was shown convex,
 *   [7] feas = max_j max(|(Jx - Ju K_j) Pz_j|, |Hn_{j+1} (A - B K_j) Pz_j|), taken inside each stage (0 when status >= 2),
 *   [8] sum_j c_j, [9] max_j c_j (the given c_N not counted), [10] / [11] smallest accepted / largest rejected pivot of the rank decisions, as in the ctg entry.
 * TMPC_E_ARG: N < 1, nph < 1, phases NULL with nph != p, a phase outside 0 .. p-1, terminal not 0 / 1, nr < ng, rank_tol <= 0, NULL outputs, (host entry) ncnt
 * outside 0 .. nr - ng.  TMPC_E_UNSUPPORTED (before the device is touched): nx + mb > TMPC_LQR_NMAX, (nx, mb, nr) beyond the 160 KB LDS layout of the ctg
 * entry, nph > 65535. */
int tmpc_horizon_lqr_batch_host(int nb, int p, int nx, int mb, int nr, int ng, int N, int nph, const int32_t* phases, int terminal, const double* A,
                                const double* B, const double* H, const double* J, const int32_t* ncnt, const double* Pf, double rank_tol, double* K0,
                                double* Pi0, double* Hn0, int32_t* cnt0, double* Kall, int32_t* cntall, double* info);
int tmpc_horizon_lqr_batch_device(int nb, int p, int nx, int mb, int nr, int ng, int N, int nph, const int32_t* phases, int terminal, const double* A,
                                  const double* B, const double* H, const double* J, const int32_t* ncnt, const double* Pf, double rank_tol, double* K0,
                                  double* Pi0, double* Hn0, int32_t* cnt0, double* Kall, int32_t* cntall, double* info);

/* Closed-loop rollouts of a phase-indexed feedback law u = -K_k x on the p-periodic model (tmpc_closed_loop.h; the LQ content of the reference's
 * closed_loop_tools.closed_loop_sim: the first-order loop -- the active set is fixed (its changes: tmpc_mpc_qp_batch_*), the nonlinear plant is not simulated).  ns initial states per
 * problem walk t = 0 .. T-1 over the stages k = (k0 + t) mod p, one launch for the whole batch:
 *     u_t = -K_k x_t,  z_t = [x_t; u_t],  l_t = 1/2 z_t' H_k z_t,  lc_t = 1/2 z_t' Hc_k z_t,  rowres_t = max|J_k z_t| over the first r_k = ng + ncnt_k rows,
 *     subres_t = max|Hn_k x_t| over all nx rows (rows beyond c_k are zero),  x_{t+1} = A_k x_t + B_k u_t.
 * Inputs: A, B as above, K [nb][p][mb][nx] (any phase-indexed law: the K of the periodic entries, the K0 of the horizon entries over all phases),
 * X0 [nb][ns][nx]; optional (NULL: absent) H, Hc [nb][p][n][n], J [nb][p][nr][n] with ncnt int32 [nb][p] (NULL: ng rows at every stage; J NULL exactly when
 * nr = 0), Hn [nb][p][nx][nx].  Outputs, TIME-MAJOR (the stores of a step are contiguous; the Python layer returns permuted views): optional X [nb][T+1][ns][nx],
 * U [nb][T][ns][mb], l, lc, rowres, subres [nb][T][ns] (each needs its input), sums [nb][ns][2] = (sum_t l_t, sum_t lc_t) added in the order of t (NaN for an
 * absent cost); required XT [nb][ns][nx] = x_T and info [nb][ns][4]:
 *   [0] status: 0 done, 3 non-finite (a non-finite value met in A, B, K, X0, H, Hc, J or Hn, or overflow during the rollout); there are no other statuses.
 *       Such a state stops at the first step t that produced a non-finite u_t, l_t, lc_t, rowres_t, subres_t or x_{t+1} (step 0 for a non-finite x_0): its
 *       entries of U, l, lc, rowres, subres from t on, of X from t + 1 on, XT and sums are NaN.  One state never affects another;
 *   [1] steps finished (T when status = 0), [2] max |x_t| over t = 0 .. steps finished (NaN for a non-finite x_0), [3] reserved (0).
 * The numbers of a state do not depend on ns or on the other states of the call (fixed order of accumulation), and the host entry stages through device
 * buffers and runs the same kernel.  TMPC_E_ARG: nb, p, nx, mb, ns, T < 1, k0 outside 0 .. p-1, nr < ng, J / nr mismatch, ncnt without J, an output without
 * its input, NULL A, B, K, X0, XT, info, (host entry) ncnt outside 0 .. nr - ng.  TMPC_E_UNSUPPORTED (before the device is touched): nx + mb > TMPC_LQR_NMAX,
 * (nx, mb, nr) beyond 160 KB of LDS for a tile of one state (every n <= 64 fits with the nr the ctg entry serves), more than 65535 tiles of states. */
#define TMPC_CLOSED_LOOP_INFO 4
int tmpc_closed_loop_batch_host(int nb, int p, int nx, int mb, int nr, int ng, int ns, int T, int k0, const double* A, const double* B, const double* K,
                                const double* X0, const double* H, const double* Hc, const double* J, const int32_t* ncnt, const double* Hn, double* X,
                                double* U, double* l, double* lc, double* rowres, double* subres, double* sums, double* XT, double* info);
int tmpc_closed_loop_batch_device(int nb, int p, int nx, int mb, int nr, int ng, int ns, int T, int k0, const double* A, const double* B, const double* K,
                                  const double* X0, const double* H, const double* Hc, const double* J, const int32_t* ncnt, const double* Hn, double* X,
                                  double* U, double* l, double* lc, double* rowres, double* subres, double* sums, double* XT, double* info);

/* The inequality-constrained tracking-MPC step and its receding-horizon loop on the p-periodic linear model (tmpc_mpc_qp.h; the reference's pmpc.py with
 * h(x, u) >= 0 at every stage, as closed_loop_tools.check_equivalence and closed_loop_sim exercise it): ns initial deviations per problem, for each the QP
 *     min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j) + 1/2 x_N' Pf_{k_N} x_N,   z_j = [x_j; u_j],   k = k_j = (k0 + j) mod p,
 *     s.t. x_{j+1} = A_k x_j + B_k u_j,  x_0 given,   D_k z_j <= d_k (first ndcnt_k rows of the stage),   j = 0 .. N-1,
 * solved at the steps t = 0 .. T-1 from the phase (k0 + t) mod p; u_0 is applied and x <- A_k x + B_k u_0 (the linear plant), one launch for the whole batch.
 * Not served (there are no arguments for them): nt > nx; the nonlinear plant inside the launch (a caller steps it with one launch per step and a shifted guess).
 * Warm starts between the steps and from a guess: the tmpc_mpc_qp_warm_batch_* entries below.
 * Soft rows (exact L1 slack penalties, the reference's `usc`): the tmpc_mpc_qp_soft_batch_* entries below.  Equality rows J z = r and the terminal
 * constraint Tx x_N = 0 (the reference's g and p_operator): the tmpc_mpc_qp_eq_batch_* entries below.  The affine problem (a dynamics offset, a linear
 * terminal cost, a terminal right-hand side, a plant that is not the model, a disturbance): the tmpc_mpc_qp_aff_batch_* entries below.  Quadratic slack
 * penalties (1/2 Z e^2 alone or beside the L1 term): the tmpc_mpc_qp_quad_batch_* entries below.
 * Method: primal-dual interior point with Mehrotra's predictor-corrector, started infeasible, the Newton system solved by a Riccati pass with a Cholesky
 * factorisation per stage; the stop rule is r_p <= tol, r_d <= tol, mu <= 1e-3 tol max(1, max lam), residuals relative to the scale of the problem (stated
 * in tmpc_mpc_qp.h and in tests/mpc_qp_reference.py).  H is used as (H + H') / 2, likewise Pf.
 * Inputs: A, B, H as above; optional (NULL: zero) q [nb][p][n], Pf [nb][p][nx][nx]; D [nb][p][nd][n], d [nb][p][nd] (both NULL exactly when nd = 0: the plain
 * horizon-N LQ problem), ndcnt int32 [nb][p] (NULL: all nd rows); X0 [nb][ns][nx]; tol > 0, max_iter >= 1 (the reference's defaults: 1e-10, 60).
 * Outputs: required U0 [nb][ns][mb] (the first input of step 0), XT [nb][ns][nx] = x_T, info [nb][ns][8]; optional (NULL: not written), the logs TIME-MAJOR as
 * in the closed-loop entry: X [nb][T+1][ns][nx], U [nb][T][ns][mb], iters, nact int32 [nb][T][ns] (iterations of the step; rows of stage 0 with lam > s),
 * hres [nb][T][ns] = max(D z - d) of the applied step (-inf at a stage without rows); and the open-loop solution of the QP of step 0: Xol [nb][ns][N+1][nx],
 * Uol [nb][ns][N][mb], Lam [nb][ns][N][nd] (rows beyond ndcnt zero).  info:
 *   [0] status: 0 converged at every step; 1 max_iter reached at some step (an infeasible instance ends here); 2 a stage matrix S = R + B' Pi B + ... not positive
 *       definite (the problem is not convex along the path, e.g. an indefinite H); 3 non-finite.  Such an instance stops at the step t that met it: U, hres from
 *       t on, X from t + 1 on, XT (and U0, Xol, Uol, Lam when t = 0) are NaN, nact from t on and iters beyond t are -1.  One instance never affects another;
 *   [1] steps finished (T when status = 0), [2] / [3] total / largest iteration count of the steps, [4] mu, [5] primal and [6] dual residual at the last stop
 *   test, [7] smallest pivot (R_cc^2) of the Cholesky factorisations.
 * The numbers of an instance do not depend on ns, on the other instances or on the workspace slot it ran in (fixed order of accumulation); the host entry stages
 * through device buffers and runs the same kernel.  Workspace: the library keeps min(nb ns, 512) slots of
 * 8 (2 (N+1) n + 6 N nd + N nx + N mb (n+1)) bytes per thread, fewer slots where that would exceed 1 GiB.
 * TMPC_E_ARG: nb, p, nx, mb, N, ns, T < 1, nd < 0, k0 outside 0 .. p-1, D / d / nd mismatch, ndcnt without D, tol <= 0, max_iter < 1, NULL A, B, H, X0, U0, XT,
 * info, (host entry) ndcnt outside 0 .. nd.  TMPC_E_UNSUPPORTED (before the device is touched): nx + mb > TMPC_LQR_NMAX, (nx, mb, nd) beyond 160 KB of LDS. */
#define TMPC_MPC_QP_INFO 8
int tmpc_mpc_qp_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                           const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol, int max_iter,
                           double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres, double* Xol, double* Uol,
                           double* Lam);
int tmpc_mpc_qp_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                             const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                             int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres, double* Xol,
                             double* Uol, double* Lam);

/* The same step and loop with SOFT rows (the reference's preprocessing.add_mpc_slacks: h + usc >= 0, usc >= 0, cost scost' usc): the 31 arguments of the entries
 * above, then
 *   penalty [nb][p][nd]: +inf a hard row D_i z <= d_i, a finite c > 0 the soft row D_i z - e_i <= d_i, e_i >= 0 with the cost c e_i at every stage of the horizon
 *                        (hard and soft rows mix freely; ndcnt keeps its meaning).  NULL: every row hard -- the hard kernel runs, Eol and nviol are zero;
 *   Eol [nb][ns][N][nd], optional: the open-loop slacks e of step 0 (0 on hard rows and beyond ndcnt; NaN when step 0 failed);
 *   nviol int32 [nb][T][ns], optional, time-major: rows of stage 0 with e > nu at the applied step (nu = c - lam the multiplier of e >= 0); -1 from a failed step on.
 * The slack and its multiplier are eliminated per row inside the interior-point iteration (tmpc_mpc_qp.h), the stage matrices keep their size; the rules of the
 * start, mu and the stop test are stated there and in tests/mpc_qp_soft_reference.py.  info, statuses and failure isolation as above; hres = max(D z - d) is
 * positive when a soft row of the applied step is violated, nact stays lam > s.  Workspace per slot: 32 N nd bytes more than above.
 * TMPC_E_ARG, besides the above: penalty with nd = 0; (host entry) a penalty <= 0 or NaN, named in the message.  On the device entry such a penalty makes the
 * instances of that problem status 3 before their first step.  TMPC_E_UNSUPPORTED: the soft layout (24 nd bytes of LDS more) beyond 160 KB, with the byte count. */
int tmpc_mpc_qp_soft_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres, double* Xol,
                                double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol);
int tmpc_mpc_qp_soft_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                  const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                  int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                  double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol);

/* The same step and loop with EQUALITY rows at every stage and a TERMINAL constraint (the reference's pmpc.py: g(x, u) = 0 and p_operator(x_N - x_ref) = 0):
 *     J_k z_j = r_k (first necnt_k rows of the stage),  j = 0 .. N-1,      Tx_{k_N} x_N = 0,  k_N = (k0 + N) mod p.
 * The 34 arguments of the soft entries (penalty NULL: every inequality row hard), then
 *   ne, J [nb][p][ne][n] (NULL exactly when ne = 0), r [nb][p][ne] (NULL: zero), necnt int32 [nb][p] (NULL: all ne rows);
 *   nt, Tx [nb][p][nt][nx], indexed by k_N like Pf: nt = 0 and Tx NULL: no terminal rows; nt = -1 and Tx NULL: x_N = 0 (Tx = I); 1 <= nt <= nx with Tx;
 *   optional outputs Nu [nb][ns][N][ne] and NuT [nb][ns][nt] (nx entries for nt = -1): the multipliers of the rows in the open-loop solution of step 0 (free sign;
 *   rows beyond necnt zero; NaN when step 0 failed); eres [nb][T][ns], time-major: max|J z_0 - r| of the applied stage (0 at a stage without rows; NaN from a
 *   failed step on).
 * An equality row is a hard row without a slack: a multiplier of free sign, the constant barrier weight 1 / rho = 1e12, no step-length limit, no part in mu or
 * the corrector; the terminal rows enter the Riccati pass where it starts (tmpc_mpc_qp.h; tests/mpc_qp_eq_reference.py states the same rules).  r_p of the stop
 * rule also takes max|J z - r| / max(1, |r|) and max|Tx x_N| / max(1, max|x|).  An instance whose rows cannot be met (N mb too short to reach Tx x_N = 0, a
 * stage-0 row on x_0 alone that x_0 violates) ends with status 1.  With ne = 0 and nt = 0 the entries above run (the same bits), eres is zero.
 * Workspace per slot: 8 (2 N ne + nt) bytes more; LDS: 8 ne (ld + 3) bytes more, ld = (n + 1) | 1.
 * TMPC_E_ARG, besides the above: ne < 0, J / ne mismatch, r or necnt without J, nt < -1, Tx / nt mismatch, (host entry) necnt outside 0 .. ne.
 * TMPC_E_UNSUPPORTED: nt > nx; the layout with the equality rows beyond 160 KB, with the byte count. */
int tmpc_mpc_qp_eq_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                              const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                              int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                              double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                              const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres);
int tmpc_mpc_qp_eq_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres);

/* The same step and loop on the AFFINE problem (the reference's controller in absolute coordinates, an estimated constant disturbance, an SQP subproblem):
 *     x_{j+1} = A_k x_j + B_k u_j + c_k,   terminal cost 1/2 x_N' Pf x_N + qf_{k_N}' x_N,   Tx_{k_N} x_N = t_{k_N},
 * and in the loop the plant x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t, k = (k0 + t) mod p.  The 43 arguments of the eq entries, then, each optional (NULL):
 *   offset [nb][p][nx]         c, indexed by the phase like A;
 *   qf [nb][p][nx]             indexed by k_N like Pf (legal without Pf);
 *   terminal_rhs [nb][p][nt]   t, indexed by k_N like Tx (nx entries for nt = -1: x_N = t);
 *   Ap [nb][p][nx][nx], Bp [nb][p][nx][mb]   the plant (both or neither; NULL: the model A, B);   cp [nb][p][nx]: its offset (NULL: the model's offset);
 *   W [nb][ns][T][nx]          the disturbance of every step, unknown to the controller.
 * XT is the plant's state after T steps; with T = 1 and no plant it is A x_0 + B u_0 + c.  hres, eres, nact, nviol stay functions of the applied z_0 of the
 * model's QP.  The iteration is the one of the eq entries with r_dyn = [A B] z + c - x+, pi_N = Pf x_N + qf + Tx' nu_T and the terminal residual Tx x_N - t
 * (tmpc_mpc_qp.h; tests/mpc_qp_affine_reference.py); the stop rule takes max|Tx x_N - t| / max(1, max|x|), and |c|, |t| enter no scale.  The kernels are
 * AFF instantiations of the two EQ kernels with their LDS layout and workspace; a call without rows runs them with ne = nt = 0.  With all seven NULL the eq
 * entry runs (the same bits).  A non-finite entry of the new arrays ends that instance with status 3 at the step that meets it (W_t, Ap, Bp, cp: at step
 * t + 1, X[t + 1] holds the non-finite state); a t that cannot be reached ends with status 1.
 * TMPC_E_ARG, besides the above: terminal_rhs with nt = 0, Ap without Bp or Bp without Ap. */
int tmpc_mpc_qp_aff_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                               const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                               int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                               double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                               const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                               const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W);
int tmpc_mpc_qp_aff_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                 const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                 int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                 double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                 const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                                 const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W);

/* The same step and loop with QUADRATIC slack penalties (the Zl / Zu of an OCP-QP beside its zl / zu): the 50 arguments of the aff entries, then
 *   penalty2 [nb][p][nd]: the L2 weight Z >= 0 of every row beside its L1 weight c = penalty.  Per row of a stage:
 *     c = +inf, Z = 0     a hard row;
 *     c > 0,    Z = 0     the soft row of the soft entries: their statements, their bits;
 *     c > 0,    Z > 0     D_i z - e <= d_i, e >= 0, cost c e + 1/2 Z e^2: two complementarity pairs, stationarity in e is c + Z e - lam - nu = 0;
 *     c = 0,    Z > 0     pure quadratic: D_i z - e <= d_i, cost 1/2 Z e^2, ONE pair (e = lam / Z >= 0 by itself): a hard row whose dual regularisation
 *                         rho + 1 / Z is exact instead of vanishing.
 * penalty is required with penalty2 (all zeros: every row pure quadratic).  Eol holds the slack of every soft row (lam / Z on a pure row); nviol counts the
 * two-pair rows with e > nu and the pure rows with lam > s (on a pure row active means violated); nact stays lam > s and hres max(D z - d).  The rules of the
 * iteration are stated in tmpc_mpc_qp.h and in tests/mpc_qp_quad_reference.py.  The kernels are QUAD instantiations of the plain soft kernel (a call without
 * equality, terminal or affine arguments) and of the soft AFF kernel (every other call); Z of the stage takes 8 nd bytes of LDS after the soft layout, the
 * workspace is the soft one.  With penalty2 NULL the aff entry runs (the same bits).
 * TMPC_E_ARG, besides the above: penalty2 without penalty; (host entry) a penalty2 that is negative, non-finite or NaN, or non-zero on a hard row; a penalty
 * that is negative or NaN, or 0 beside penalty2 = 0: each named in the message.  On the device entry any of these makes the instances of that problem status 3
 * before their first step.  TMPC_E_UNSUPPORTED: the layout with Z beyond 160 KB, with the byte count. */
int tmpc_mpc_qp_quad_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                                const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W,
                                const double* penalty2);
int tmpc_mpc_qp_quad_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                  const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                  int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                  double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                  const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                                  const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W,
                                  const double* penalty2);

/* The same step and loop WARM-STARTED (the reference's Pmpc.step always starts from its shifted previous solution): the 51 arguments of the quad entries, then
 *   warm_flags: bit 0 every step t > 0 of the loop starts from the shifted iterate of step t - 1; bit 1 step 0 starts from the guess below; bit 2 (only with
 *               bit 1) the guess is shifted by one stage first (it comes from the previous phase);  0: the quad entry runs (the same bits), warmlog is zero;
 *   warm_floor: delta > 0 of the floors (1e-2 is the default of the Python calls);
 *   the guess, exactly with bit 1, Xg and Ug at the least, the others NULL where the problem has none (NULL: zeros): Xg [nb][ns][N+1][nx], Ug [nb][ns][N][mb],
 *               Lamg [nb][ns][N][nd], Eg [nb][ns][N][nd] (only with penalty), Nug [nb][ns][N][ne], NuTg [nb][ns][nt] -- what an earlier call returned as Xol,
 *               Uol, Lam, Eol, Nu, NuT;
 *   warmlog int32 [nb][T][ns], optional, time-major: 0 the step started cold, 1 the warm start delivered it, 2 the warm attempt failed and the cold restart
 *               delivered it, -1 from a failed step on.
 * The rule (tmpc_mpc_qp.h; tests/mpc_qp_warm_reference.py states the same one).  Shift: new stage j takes old stage j + 1 for j <= N - 2, x_0 is the measured
 * state, u_{N-1} repeats the old last input, x_N = A_k x_{N-1} + B_k u_{N-1} (+ c_k) at the phase of the new last stage; multipliers and slacks shift the
 * same way, the new last stage gets zeros before the floors, nu_T is kept.  Without a shift everything is as given and x_0 is replaced.  Floors: a hard row
 * takes s = max(d - D z, delta), lam = max(lam, delta); an L1 or L1 + L2 row e = max(e, delta), lam = clip(lam, delta, c + Z e - delta),
 * nu = c + Z e - lam (lam = nu = (c + Z e) / 2 when c + Z e < 2 delta), s = max(d - D z + e, delta); a pure quadratic row lam = max(lam, delta),
 * s = max(d - D z + lam / Z, delta); equality and terminal multipliers are free.  s and nu are derived, never read.  Fallbacks: an instance whose guess holds
 * a non-finite entry starts cold (a failed predecessor returns NaN); a warm-started step that ends with status 1 or 2 is solved again from the cold start
 * within the step and iters counts both attempts, so an infeasible instance costs two runs of max_iter; status 3 is not retried.  The kernels are WARM
 * instantiations beside each of the eight, with their LDS layout and workspace.
 * TMPC_E_ARG, besides the above: warm_flags outside 0 .. 7 or bit 2 without bit 1; guess arrays without bit 1, or bit 1 without Xg and Ug; Lamg with nd = 0,
 * Eg without penalty, Nug with ne = 0, NuTg with nt = 0; warm_floor <= 0, non-finite or NaN. */
int tmpc_mpc_qp_warm_batch_host(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                                const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W,
                                const double* penalty2, int warm_flags, double warm_floor, const double* Xg, const double* Ug, const double* Lamg,
                                const double* Eg, const double* Nug, const double* NuTg, int32_t* warmlog);
int tmpc_mpc_qp_warm_batch_device(int nb, int p, int nx, int mb, int nd, int N, int ns, int T, int k0, const double* A, const double* B, const double* H,
                                  const double* q, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* X0, double tol,
                                  int max_iter, double* U0, double* XT, double* info, double* X, double* U, int32_t* iters, int32_t* nact, double* hres,
                                  double* Xol, double* Uol, double* Lam, const double* penalty, double* Eol, int32_t* nviol, int ne, const double* J,
                                  const double* r, const int32_t* necnt, int nt, const double* Tx, double* Nu, double* NuT, double* eres, const double* offset,
                                  const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W,
                                  const double* penalty2, int warm_flags, double warm_floor, const double* Xg, const double* Ug, const double* Lamg,
                                  const double* Eg, const double* Nug, const double* NuTg, int32_t* warmlog);

/* The local feedback gain of a SOLVED MPC step (tmpc_mpc_qp_gain.h): at a strictly complementary solution of the QP of tmpc_mpc_qp_*_batch the first input is
 * locally affine in x_0, u_0(x_0 + dx) = u_0 - K0 dx, and K0 is the first gain of the equality-constrained LQ problem that keeps the active set.  One backward
 * pass j = N-1 ... 0 over the stages k = (k0 + j) mod p per (problem, instance), the constraint-to-go stage of the horizon entry, so any active set is served
 * (more active rows than inputs, rows on the state alone, dependent rows) and no row enters at a penalty weight.
 * Inputs: nb, p, nx, mb, nd, ne, nt, N, ns, k0 and A, B, H, Pf, D, ndcnt, d, penalty, penalty2, J, necnt, Tx as in the MPC QP entries (H and Pf are used as
 * their symmetric parts; penalty NULL: every row hard; penalty2 NULL: zero); terminal: 0 none, 1 x_N = 0, 2 the rows Tx [nb][p][nt][nx] of phase (k0 + N) mod p
 * (orthonormalised by the compression of the stage); the solution X [nb][ns][N+1][nx], U [nb][ns][N][mb], Lam [nb][ns][N][nd], Eps [nb][ns][N][nd] (NULL: zero)
 * as the QP entries return Xol, Uol, Lam, Eol; cls_in int32 [nb][ns][N][nd] or NULL; rank_tol as in the ctg entry.
 * Class of row (j, i), with g = d_i - D_i z_j (cls_in replaces it; values other than 1, 2 count as 0, as does 2 on a row without penalty2):
 *     hard row (penalty inf): s = g;  1 if lam > s, else 0.      pure quadratic (penalty 0, Z = penalty2 > 0): s = g + lam / Z;  2 if lam > s, else 0.
 *     0 < penalty < inf: s = g + e, nu = penalty + Z e - lam;  0 if not lam > s; else, violated (e > nu): 2 if Z > 0, 0 if Z = 0; not violated: 1.
 *     rows beyond ndcnt, and penalty 0 beside penalty2 0 (no row kind; s = g): 0.      0 free: the row drops out; 1 equality: D_i dz_j = 0; 2 quadratic: the stage Hessian gains Z_i D_i' D_i.
 * The rows J_k (first necnt_k) and the terminal rows always hold.  q, r, offset, qf and terminal_rhs enter only through the solution.
 * Outputs per (problem, instance): K0 [nb][ns][mb][nx], Pi0, Hn0 [nb][ns][nx][nx], cnt0 int32 [nb][ns], info [nb][ns][12] with the slots of the horizon entry
 * (K0, Pi0 projected on Hn0 dx = 0, the directions in which the active set can be kept); optional (NULL: not written, the rest keeps its bits): cls int32
 * [nb][ns][N][nd]; strict [nb][ns] = min over the complementarity pairs (lam, s) and, on two-pair rows, (e, nu) of |a - b| / max(|a|, |b|) -- near 1: the
 * active set is unambiguous, near 0: a weakly active row, the derivative is one-sided and the result means nothing --; Kall [nb][ns][N][mb][nx], cntall int32
 * [nb][ns][N]; dX [nb][ns][N+1][nx][nx], dU [nb][ns][N][mb][nx], the open-loop sensitivities Phi_0 = Pz_0, dU_j = -K_j Phi_j, Phi_{j+1} = (A - B K_j) Phi_j
 * (together, and with Kall).  An instance whose solution holds a non-finite entry ends with status 3; with status >= 2 K0, Pi0, strict, dX, dU are NaN, Hn0
 * zero, and the unfinished stages of Kall / cntall / cls hold NaN / -1 / -1.  One instance never affects another, and its numbers do not depend on ns.
 * The host entry stages through device buffers and runs the same kernel.  Not returned: sensitivities of the multipliers.
 * TMPC_E_ARG: sizes < 1 (nd, ne, nt < 0), k0 outside 0 .. p-1, terminal not 0 / 1 / 2 or 2 without Tx / with nt < 1, NULL A, B, H, X, U, outputs,
 * nd > 0 without D, d or Lam, penalty2 without penalty, ne > 0 without J, dX without dU or Kall, rank_tol <= 0, (host entry) ndcnt / necnt out of range.
 * TMPC_E_UNSUPPORTED (before the device is touched): terminal 2 with nt > nx, nx + mb > TMPC_LQR_NMAX, the layout of the ctg entry with ne + nd rows plus nd + 1 doubles beyond 160 KB,
 * nb > 65535. */
int tmpc_mpc_qp_gain_batch_host(int nb, int p, int nx, int mb, int nd, int ne, int nt, int N, int ns, int k0, int terminal, const double* A, const double* B,
                                const double* H, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* penalty,
                                const double* penalty2, const double* J, const int32_t* necnt, const double* Tx, const double* X, const double* U,
                                const double* Lam, const double* Eps, const int32_t* cls_in, double rank_tol, double* K0, double* Pi0, double* Hn0,
                                int32_t* cnt0, double* info, int32_t* cls, double* strict, double* Kall, int32_t* cntall, double* dX, double* dU);
int tmpc_mpc_qp_gain_batch_device(int nb, int p, int nx, int mb, int nd, int ne, int nt, int N, int ns, int k0, int terminal, const double* A, const double* B,
                                  const double* H, const double* Pf, const double* D, const int32_t* ndcnt, const double* d, const double* penalty,
                                  const double* penalty2, const double* J, const int32_t* necnt, const double* Tx, const double* X, const double* U,
                                  const double* Lam, const double* Eps, const int32_t* cls_in, double rank_tol, double* K0, double* Pi0, double* Hn0,
                                  int32_t* cnt0, double* info, int32_t* cls, double* strict, double* Kall, int32_t* cntall, double* dX, double* dU);

/* The periodic optimal-control QP on the p-periodic affine model (tmpc_periodic_qp.h; the LQ case of the reference's pocp.py, the QP subproblem of its
 * sqp_method.Sqp): the orbit that the MPC entries above take as their reference.  Per problem, with N = periods p and k_j = j mod p,
 *     min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j),   z_j = [x_j; u_j],
 *     s.t. x_{j+1} = A_k x_j + B_k u_j + c_k,  j = 0 .. N-1,  x_N := x_0  (x_0 is a variable),
 *          D_k z_j <= d_k (first ndcnt_k rows of the stage),   J_k z_j = r_k (first necnt_k rows of the stage).
 * Soft and quadratic-slack rows: the tmpc_periodic_qp_soft_batch pair below.  Not served (there are no arguments for them): warm starts, a terminal cost
 * (Pf has no meaning without an end), the phase-fixing cost of pocp.py, nonlinear dynamics and the SQP outer loop.
 * Method: the interior-point iteration of the MPC entries (hard rows, equality rows at the weight 1 / rho, Mehrotra's predictor-corrector, one step length,
 * the same stop rule: tmpc_periodic_qp.h and tests/periodic_qp_reference.py state the rules).  The multiplier of x_N = x_0 is a variable of the iteration; the
 * Newton system is the Riccati pass plus a border of nx columns and one symmetric quasi-definite system of size 2 nx per iteration.
 * Inputs: A [nb][p][nx][nx], B [nb][p][nx][mb], H [nb][p][n][n] (used as (H + H') / 2); optional (NULL: zero) q [nb][p][n], offset c [nb][p][nx];
 * D [nb][p][nd][n], d [nb][p][nd] (both NULL exactly when nd = 0), ndcnt int32 [nb][p] (NULL: all nd rows; a count outside 0 .. nd is clamped to it);
 * J [nb][p][ne][n] (NULL exactly when ne = 0), r [nb][p][ne] (NULL: zero), necnt int32 [nb][p] (NULL: all ne rows; clamped to 0 .. ne); tol > 0,
 * max_iter >= 1 (the defaults of the reference statement: 1e-10, 60).
 * Outputs: required info [nb][8]; optional (NULL: not written) X [nb][N][nx] = x_0 .. x_{N-1}, U [nb][N][mb], Lam [nb][N][nd] (rows beyond ndcnt zero),
 * Nu [nb][N][ne] (free sign; rows beyond necnt zero), Pi [nb][N][nx]: the multipliers of the dynamics, Pi[0] that of x_N = x_0 and Pi[j] that of
 * x_j = A x_{j-1} + B u_{j-1} + c, with (H z_j + q + D' lam_j + J' nu_j)_x + A_j' Pi[(j + 1) mod N] = Pi[j]; res [nb][4] = (cost, hres = max(D z - d) over
 * all stages (-inf without rows), eres = max|J z - r|, per = max|A x_{N-1} + B u_{N-1} + c - x_0|).  info, the fields of the MPC entries:
 *   [0] status: 0 converged; 1 max_iter reached (contradictory rows end here); 2 a stage matrix, Pi_0 or the border's Schur complement not positive definite
 *       (not convex along the path, or no unique periodic trajectory: A = I, B = 0, c != 0 ends here -- such a problem never ends with 0); 3 non-finite.
 *       With status != 0 X, U, Lam, Nu, Pi, res are NaN.  One problem never affects another;
 *   [1] steps: 1 on success, else 0; [2] = [3] iterations; [4] mu, [5] primal and [6] dual residual at the last stop test; [7] smallest pivot of the
 *   Cholesky factorisations, those of the border included.
 * The numbers of a problem do not depend on nb, on the other problems or on the workspace slot it ran in (fixed order of accumulation); the host entry stages
 * through device buffers and runs the same kernel.  Workspace: the library keeps min(nb, 512) slots of
 * 8 (2 (N+1) n + 6 N nd + N nx + N mb (n+1) + 2 N ne + N mb nx + N nx) bytes per thread, fewer slots where that would exceed 1 GiB.  LDS: the layout of the
 * eq entries with nt = 0 plus 8 ldp (2 nx + n + mb + 10) bytes, ldp = nx | 1 (nx 24 / mb 8 / nd 16: 56144 bytes).
 * TMPC_E_ARG: nb, p, nx, mb, periods < 1, nd, ne < 0, D / d / nd mismatch, ndcnt without D, J / ne mismatch, r or necnt without J, tol <= 0, max_iter < 1,
 * NULL A, B, H, info.  TMPC_E_UNSUPPORTED (before the device is touched): nx + mb > TMPC_LQR_NMAX, the layout beyond 160 KB of LDS (with the byte count),
 * periods p beyond 32-bit indices inside a slot. */
#define TMPC_PERIODIC_QP_INFO 8
#define TMPC_PERIODIC_QP_RES 4
int tmpc_periodic_qp_batch_host(int nb, int p, int nx, int mb, int nd, int ne, int periods, const double* A, const double* B, const double* H, const double* q,
                                const double* offset, const double* D, const int32_t* ndcnt, const double* d, const double* J, const double* r,
                                const int32_t* necnt, double tol, int max_iter, double* X, double* U, double* Lam, double* Nu, double* Pi, double* info,
                                double* res);
int tmpc_periodic_qp_batch_device(int nb, int p, int nx, int mb, int nd, int ne, int periods, const double* A, const double* B, const double* H, const double* q,
                                  const double* offset, const double* D, const int32_t* ndcnt, const double* d, const double* J, const double* r,
                                  const int32_t* necnt, double tol, int max_iter, double* X, double* U, double* Lam, double* Nu, double* Pi, double* info,
                                  double* res);

/* The periodic QP with soft and quadratic-slack rows (k_periodic_qp<true> of tmpc_periodic_qp.h): the arguments of the pair above plus
 * penalty = c and penalty2 = Z, each [nb][p][nd] or NULL, read per row as the tmpc_mpc_qp_quad entries read them:
 *     c = inf (Z = 0)  the hard row;            c > 0, Z = 0  D_i z - e <= d_i, e >= 0, cost c e (exact L1);
 *     c > 0, Z > 0     cost c e + 1/2 Z e^2;    c = 0, Z > 0  cost 1/2 Z e^2, e = lam / Z (pure quadratic, one complementarity pair).
 * penalty NULL with penalty2: every row is pure quadratic (c = 0); penalty2 NULL with penalty: Z = 0.  With both NULL the call runs the kernel of the pair
 * above and writes its bits, with zeros in Eps, nviol, pcost and emax.  The slacks are eliminated per row (start values, weights, corrector terms, step length
 * and stop rule are those of the MPC entries; the border of the periodic Newton system is unchanged).  A problem whose rows contradict each other and are all
 * soft converges to the least-penalised violation instead of ending with status 1.
 * Outputs beyond those of the pair above (each or NULL): Eps [nb][N][nd], the slack of every soft row (lam / Z on a pure row, 0 on hard and absent rows);
 * nviol int32 [nb], over all N stages the two-pair rows with e > nu plus the pure rows with lam > s; res [nb][6] = (cost, hres, eres, per, pcost, emax):
 * cost is the total and includes pcost = sum c e + 1/2 Z e^2, emax = max e, hres stays max(D z - d) and is positive when a row is violated.
 * An invalid weight (c negative or NaN; Z negative or non-finite; Z != 0 on a hard row; c = 0 with Z = 0) gives that problem status 3 before its first
 * iteration.  With status != 0 the floating-point outputs are NaN and nviol is -1.
 * Workspace per slot: that of the pair above plus 8 (4 N nd) bytes.  LDS: that of the pair above plus 8 (4 nd) bytes (nx 24 / mb 8 / nd 16: 56656 bytes).
 * TMPC_E_ARG as above, and a non-NULL penalty or penalty2 with nd = 0.  TMPC_E_UNSUPPORTED as above, with the byte count of the soft layout. */
#define TMPC_PERIODIC_QP_SOFT_RES 6
int tmpc_periodic_qp_soft_batch_host(int nb, int p, int nx, int mb, int nd, int ne, int periods, const double* A, const double* B, const double* H,
                                     const double* q, const double* offset, const double* D, const int32_t* ndcnt, const double* d, const double* penalty,
                                     const double* penalty2, const double* J, const double* r, const int32_t* necnt, double tol, int max_iter, double* X,
                                     double* U, double* Lam, double* Eps, double* Nu, double* Pi, int32_t* nviol, double* info, double* res);
int tmpc_periodic_qp_soft_batch_device(int nb, int p, int nx, int mb, int nd, int ne, int periods, const double* A, const double* B, const double* H,
                                       const double* q, const double* offset, const double* D, const int32_t* ndcnt, const double* d, const double* penalty,
                                       const double* penalty2, const double* J, const double* r, const int32_t* necnt, double tol, int max_iter, double* X,
                                       double* U, double* Lam, double* Eps, double* Nu, double* Pi, int32_t* nviol, double* info, double* res);

/* Accumulated hipEvent timings since the last call (ms) when TMPC_FLAG_PROFILE is set, 16 doubles:
 * out[0] stage_pre+ctrl, [1] schur assembly, [2] block factorisation (all kernels of tmpc_cr.h's factor phase), [3] predictor
 * pass, [4] corrector pass + update, [5] number of factorisation phases (= IPM iterations of the chunks), [6] total ms of the
 * convexify calls, [7] IPM iterations (max over chunk, summed over chunks), [8] problem-factorisations (sum over the phases of
 * the problems still iterating), [9] / [10] / [11] ms inside k_cr_potrf / k_cr_trsm / k_cr_update (fp64), [12] lanes of the handle, [13] problem-factorisations
 * whose Schur-complement updates ran in single precision (TMPC_TUNE_LOWP_SWITCH), [14] ms inside k_cr_update_dma_f32.
 * Counted with or without the flag: [15] problems solved through the one-launch kernel of TMPC_TUNE_PERSISTENT (k_ipm_small) since the last call. */
int tmpc_get_profile(tmpc_handle* h, double* out16);

/* Optimality certificate of the LAST wave solved (nb <= chunk, plain Step 1 model): the DUAL iterate of the interior-point method,
 * i.e. the multipliers of the 2p LMIs of convexifier.py:304-306 in the scaled problem
 *     min tau  s.t.  S1_k = M_k - I >= 0,  S2_k = tau I - M_k >= 0,  alpha - 1e-8 >= 0,   M_k = alpha s H_k + calH_k(Pbar):
 * X1, X2 [nb][p][n][n] (>= 0) and scal [nb][4] = (x0, tau, alpha, mu_target).  For a dual-feasible triple (sum_k tr X2_k = 1,
 * sum_k <s H_k, X1_k - X2_k> + x0 = 0, calH*(X1 - X2) = 0) weak duality gives  sum_k tr X1_k + 1e-8 x0  <=  kappa* (the optimal
 * max condition number), so together with the primal point (P, alpha, kappa outputs: cond(Hc_k) <= kappa) a caller can bound the
 * optimality gap of kappa without trusting this solver (tests/test_gpu_parity.py::test_dual_certificate does it in numpy).
 * Any pointer may be NULL.  Early-exit members (already convex) hold no meaningful dual. */
int tmpc_get_dual_host(tmpc_handle* h, int nb, double* X1, double* X2, double* scal);
/* The dual side of the stage-local multipliers of the LAST wave solved by a handle with G / C rows (Step 1 with G, Step 2 model), scaled problem, for the
 * same solver-independent certificate (tests/test_gpu_parity.py::test_dual_certificate_with_multipliers):
 *   phi [nb][p][nr]  the multipliers s*[Fg_k; F_k] (nr = ng + nc of the handle; entries beyond a stage's row count are padding),
 *   z   [nb][p][nr]  their duals (phi_i >= 0  <->  z_i >= 0),
 *   aX  [nb][p][2][TMPC_ARROW_LD][TMPC_ARROW_LD], at [nb][p][2]   Step 2 with rho > 0 only (else pass NULL): the primal blocks X_e of the arrow LMIs of the (up to) two norm terms
 *                    per stage (leading (m_e + 1) x (m_e + 1) part valid; term 0 = the rows of G if ng > 0, then the rows of C_k) and the epigraph variables t_e.
 * X1, X2, x0, tau, alpha, mu_target come from tmpc_get_dual_host.  Any pointer may be NULL. */
int tmpc_get_dual_con_host(tmpc_handle* h, int nb, double* phi, double* z, double* aX, double* at);

/* Per-iteration diagnostics of the LAST chunk solved: out[nb][80][10] = (iteration, phase, mu, tau, pinf, dinf,
 * primal step, dual step, relative output change of the step, cumulative shifted pivots); nb <= chunk. */
int tmpc_get_trace(tmpc_handle* h, int nb, double* out);

const char* tmpc_last_error(void);
const char* tmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TUNEMPC_HIP_H */
