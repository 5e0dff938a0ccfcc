/*
 * tunempc_hip_debug.h -- unit-test and diagnostic entry points of libtunempc_hip.so.
 *
 * NOT part of the drop-in boundary (that is tunempc_hip.h): the tests call the building blocks of the kernels through the
 * same shared library, and the scripts under scripts/ read back raw workspace arrays.  Nothing here has a counterpart in the
 * reference.
 */
#ifndef TUNEMPC_HIP_DEBUG_H
#define TUNEMPC_HIP_DEBUG_H

#include "tunempc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug bit for tmpc_set_options(flags): the solve stops after ASSEMBLING the Schur system of the first iteration (of iteration k after
 * tmpc_debug_set_stop_iteration(h, k)), which then sits unfactored in the workspace for tmpc_debug_get_array (tests/test_gpu_t3_kernels.py,
 * tests/test_gpu_schur_assembly.py).  The outputs of such a call are NOT a solution -- never set it in product code. */
#define TMPC_DEBUG_FLAG_STOP_ASSEMBLED 8
/* Debug bit: no relative lift of the Schur diagonal after frozen pivots (REG_MAX = 0): frozen pivots in the centering phase then go straight to the
 * route 'back mu_t off and take the step of this factorisation' (ctrl_backoff_before_rhs / k_ctrl_c), which the lifts make rare in practice
 * (tests/test_gpu_hard_targets.py::test_backoff_step_is_taken).  Never set it in product code. */
#define TMPC_DEBUG_FLAG_NO_LIFT 16
/* Debug bit: the register-staged factorisation kernels (k_cr_potrf / k_cr_trsm / k_cr_update: the path of blocks wider than 320) for every block
 * size, instead of the LDS-DMA kernels -- keeps that path under test at small shapes. */
#define TMPC_DEBUG_FLAG_NO_DMA 32
/* Debug bit: the generic per-stage kernels of stage blocks wider than 32 (tmpc_big.h; with them the <true> forms of the multiplier and Step 3 kernels) also at n <= 32, so that they can be
 * compared with the tuned kernels on the same inputs. */
#define TMPC_DEBUG_FLAG_GENERIC_STAGE 64
/* Debug bit: only the multiplier kernels (csrc/tmpc_phi.h) take their forms for stage blocks wider than 32 (k_phi_pre<true, *>, k_phi_rhs<true>, kb_phi_dm + k_phi_dir<true>)
 * at n <= 32; the stage kernels stay the tuned ones, so both forms see the same inputs bit for bit and must return the same bits (tests/test_gpu_phi_kernels.py).
 * In a Step 3 call the bit also selects k_t3_schur<true> (csrc/tmpc_t3.h) at n <= 32, under the same rule (tests/test_gpu_t3_kernels.py). */
#define TMPC_DEBUG_FLAG_GENERIC_ROWS 128

/* C (M x N) <op> A (M x K) * B (N x K)' with the fp64 MFMA tile GEMMs of the factorisation; mode 0: C -= AB', 1: C = AB', 2: C = -AB'.
 * mode + 0: the register-staged core (tmpc_factor.h, one workgroup walks all tiles); + 16: the LDS-DMA tile core (tmpc_gemm_dma.h, one
 * workgroup per 64 x 64 tile); + 32: the LDS-DMA core with K split into two operand pairs of K/2 as one stream.  lower != 0: only the
 * part on and below the diagonal (register-staged: 64 x 64 tiles and the waves that reach the diagonal; LDS-DMA: 16 x 16 blocks).
 * All dims multiples of 16 (K of 32 for + 32). */
int tmpc_debug_gemm_nt(tmpc_handle* h, double* C, const double* A, const double* B, int M, int N, int K, int mode, int lower);

/* Factor + solve one SPD block-cyclic-tridiagonal system with the cyclic-reduction kernels (tmpc_cr.h):
 * D [p][d][d] diagonal blocks, Ccpl [p][d][d] with Ccpl[k] = T[block k, block k+1 mod p], rhs/x [p][d]. */
int tmpc_debug_block_solve(tmpc_handle* h, int p, int d, const double* D, const double* Ccpl, const double* rhs, double* x, int32_t* nshift);

/* The block factorisation and its substitutions AS THE SOLVER DRIVES THEM (cr_factor / cr_solve, dd_factor / dd_solve), with the factor read back:
 * nb distinct systems in one workspace, an ordered problem list (any subset of 0..nb-1, uploaded as the compacted list of the kernels), a per-problem
 * precision, the pass, the forward sweep fused into the factorisation or not.  Unit tests of the float32 and double-double kernels (tests/test_gpu_factor_kernels.py).
 * The no-MFMA flag and TMPC_DEBUG_FLAG_NO_DMA of the handle are honoured (the latter at every block size, unlike tmpc_debug_block_solve).
 * A combination the solver itself never runs (float32 without the LDS-DMA kernels or outside 64 < dp <= 320, a fused sweep at p = 1 or on the small-block kernel,
 * float32 or a fused sweep in double-double) is TMPC_E_ARG, never a quiet change of path. */
#define TMPC_DEBUG_FACTOR_PASS1 1       /* pass 1: three right-hand sides per problem, interleaved as in W3 [p][dp][3]; else pass 2: one, in Z [p][dp] */
#define TMPC_DEBUG_FACTOR_FUSE_FWD1 2   /* pass 1 only: the forward sweep rides inside the factorisation (cr_factor fuse_fwd1, cr_solve skip_fwd) */
#define TMPC_DEBUG_FACTOR_LOWP_TRSM 4   /* DF_LOWP_TRSM for this call: the problems with lowp[b] != 0 also solve in float32 (k_cr_trsm_dma_f32) */
#define TMPC_DEBUG_FACTOR_DD 8          /* dd_factor + dd_solve on hi (+ lo) words; right-hand sides are fp64 numbers (dd_solve clears their low words) */
typedef struct {
  /* in: D, Ccpl [nb][p][d][d] (Ccpl[b][k] = T_b[block k, block k+1 mod p]), rhs [nb][p][d][nc] with nc = 3 (pass 1) or 1; Dlo / Clo: low words (double-double
   * only; NULL = zero); list [count]; lowp [nb]: 1 = this problem's updates in float32 (I_LOWP; NULL = none) */
  const double *D, *Ccpl, *Dlo, *Clo, *rhs;
  const int32_t *list, *lowp;
  /* out, every problem of the batch whether listed or not, the padded device images as they are (any pointer may be NULL): D (-> L), O (edge slots), F (fill
   * slots) [nb][p][dp][dp]; O32 [nb][2p][dp][ld32] (calls with a float32 problem only); Ddiag [nb][p][dp]; X [nb][p][dp][nc]; the low words of D, O, F, X
   * (double-double only); nshift [nb]; dims [4] = dp, ld32, nc, 1 if O32 exists; orient [p]: 0 = edge slot k holds T[k+1,k], 1 = T[k,k+1] */
  double *oD, *oO, *oF, *oDdiag, *oX;
  float* oO32;
  double *oDl, *oOl, *oFl, *oXl;
  int32_t *nshift, *dims, *orient;
} tmpc_debug_factor_io;
int tmpc_debug_block_factor(tmpc_handle* h, int nb, int p, int d, int count, int mode, const tmpc_debug_factor_io* io);
/* How many two-edge items (TMPC_TUNE_TRSM_PAIR: problem x node with both edges x strip) the last tmpc_debug_block_factor / tmpc_debug_factor_bench of this
 * process launched in k_cr_trsm_dma_f32 -- counted on the host from the schedule and the problem list where cr_factor launches the kernel, no device counter.
 * 0: the key is off, no float32 solve ran, or no node of the schedule has two edges (p = 2). */
long long tmpc_debug_last_trsm_pairs(void);

/* The elimination schedule for period p (host only, no device needed): out = [nlev, prep, nelim, nupd, nlev x (eoff, nelim,
 * uoff, nupd), nelim x 8 ints (node, na, nb, ea, eb, fill, fx, facc), nupd x 8 ints (node, e0, src0, e1, src1, 0, 0, 0),
 * p x orientation].  Returns the number of ints; call with out = NULL to size the buffer. */
int tmpc_debug_cr_schedule(int p, int32_t* out, int cap);

/* Scaled stage-local multipliers of the LAST chunk solved (row stride nr of that call): phi, their duals z and the last
 * directions, each [nb][p][nr]; any pointer may be NULL. */
int tmpc_debug_get_multipliers(tmpc_handle* h, int nb, int nr, double* phi, double* z, double* dphi, double* dz);

/* Raw workspace read-back for diagnostics, LANE 0 ONLY (a handle made with tmpc_create_ex(..., lanes = 1) and chunk >= the batch keeps a whole call there):
 * `count` doubles from `offset` of the array `which` (no bounds check beyond the pointer being allocated).  Shapes as in the workspace, B = problems of the chunk:
 *   0 psm [B,p,nz*nz+6*nz]   1 pvec [B,p,2,nr,2n+2nx]   2 Ddiag [B,p,dp]   3 D [B,p,dp,dp]   4 part [B,p,26]   5 O [B,p,dp,dp] (edge slots 0..p-1)
 *   6 F [B,p,dp,dp] (fill slots)   7 W3 [B,p,dp,3] (pass-1 right-hand sides: rhs | u_tau | u_alpha)   8 U [B,p,dp,2] (border columns tau, alpha)
 *   the iterate and the scaled data:   9 X1   10 X2   11 S1   12 S2 [B,p,n,n]   13 P [B,p,nx,nx]   14 V = [A B] [B,p,nx,n]   15 Hb = s H [B,p,n,n]
 *   the stage data of the iteration:   16 S1i   17 S2i   18 Rd1   19 Rd2   20 T1   21 T2 [B,p,n,n]
 *   what the assembly kernels read and write:   22 KF [B,p,12,nx,nx] (Kronecker factors: XXX, SIXX, KX, KS, FX, FS of LMI 1, then of LMI 2)
 *   23 adjV   24 adjE [B,p,3,nx,nx] (adjoint pieces: G = T1 - T2, Psi, PhiH)   25 Z [B,p,dp]   26 prob [B,48] (per-problem scalars: 0 tau, 1 alpha, 2 s0, 3 x0,
 *   4 mu, 5 mu_t, 6 sigma mu, ...: the P_* enum of csrc/tmpc_common.h)   27 trace [B,80,10] (row i-1: iteration i as written by its k_ctrl_c: it, phase, mu, tau,
 *   pinf, dinf, ap, ad, stepn, shifts)
 *   the direction of the iteration (pass 1: predictor, pass 2: final; a pass overwrites the one before):   28 dP [B,p,nx,nx]   29 dX1   30 dX2   31 dS1   32 dS2 [B,p,n,n]
 *   33 c1   34 c2 [B,p,n,n] (Mehrotra term sym(dX dS S^-1) of pass 1)   35 L1i   36 L2i   37 LX1i   38 LX2i [B,p,n,n] (inverse Cholesky factors of S_r and X_r, lower
 *   triangular, written by k_stage_pre)   39 Wm [B,p,4,n,n] (step-length matrices; slot 2r: L_r^-1 dS_r L_r^-T, slot 2r+1: LX_r^-1 dX_r LX_r^-T)   40 eigmin [B,p,4] (their
 *   smallest eigenvalues, or the bound -1/theta of k_eigmin's pre-test)   41 TU [B,p,dp,2] (T^-1 U of the last factorisation)
 *   the stage-local multipliers (csrc/tmpc_phi.h; handles with rows only; phi, z, dphi, dz: tmpc_debug_get_multipliers):   42 G [B,p,nr,n] (rows of [G_k; C_k] as the last host-buffer call staged them, row stride nr of that call)
 *   43 corrp [B,p,nr] (Mehrotra term dz dphi / phi of pass 1)   44 at   45 adt [B,p,2] (epigraph variables of the norm terms, their directions)
 *   46 aX   47 adX   48 acor   49 aSi   50 aLi   51 aLXi [B,p,2,AE] (arrow blocks, AE = 32 x 32 with row stride 32: X, dX, sym(dX dS S^-1), S^-1, L_S^-1, L_X^-1)
 *   52 asum [B,p,5] (<dX,S>, <X,dS>, <dX,dS>, smallest eigenvalue dual / primal of the arrow blocks)   53 prs [B,p,4,nr,nr] (Gram products g_i' X_r g_j (slots 0, 1),
 *   g_i' S_r^-1 g_j (2, 3) of handles with room for more than 32 rows per stage; absent otherwise)
 *   the regularisation T_k of Step 3 (csrc/tmpc_t3.h; handles with room for T, after a Step 3 call; m = n (n + 1) / 2 entries (a <= b) of T_k, row-major upper triangle):
 *   54 th   55 z   56 dth   57 dz [B,p,m] (theta, its dual and their directions)   58 cth [B,p,m] (Mehrotra term dz dth / th of pass 1)
 *   59 x   60 dx [B,p,m+1] (multiplier of the norm cone and its direction)   61 cq [B,p,m+1] (Mehrotra term of the cone, pass 1)   62 g [B,p,m+1] (sig s^-1 - x - cq: k_t3_rhs)
 *   63 v   64 lam [B,p,m+1] (Nesterov-Todd scaling W = beta (2 v v' - J) and lambda = W x, written by k_t3_pre)   65 t   66 dt   67 beta [B,p] (epigraph variable, its direction, beta)
 *   68 t3psi   69 t3phi [B,p,n,n] (sym(X_2 S_2^-1) and sum_r sym(X_r Hb S_r^-1): what the theta rows of the border columns read)
 * A code whose array this handle does not have is TMPC_E_ARG; so are the codes of Step 3 after a call that ran without it (a handle with room for T also serves the other models). */
int tmpc_debug_get_array(tmpc_handle* h, int which, uint64_t offset, uint64_t count, double* out);
/* The integer state, LANE 0 ONLY like tmpc_debug_get_array: `count` ints from `offset` of iprob [B,24] (per problem: 0 phase (0 main, 1 centering, 2 done), 1 iterations,
 * 5 I_NSHIFT, 9 I_SHIFT0, 12 I_REG, 13 I_CHORD, 19 I_LOWP, ...: the I_* enum of csrc/tmpc_common.h). */
int tmpc_debug_get_iprob(tmpc_handle* h, uint64_t offset, uint64_t count, int32_t* out);

/* With TMPC_DEBUG_FLAG_STOP_ASSEMBLED: stop at iteration k >= 1 instead of the first (the default, k = 1).  Iterations 1 .. k-1 run exactly as the solver runs them
 * (launch sequence: the flag turns graph replay and the persistent kernel off for the call); iteration k runs k_stage_pre, k_ctrl_a, the assembly and the pass-1
 * right-hand sides (k_stage_rhs, k_gather) and returns, so row k of the trace is not written yet.  Without the flag the value is not read.
 * The same as tmpc_debug_set_stop_point(h, k, TMPC_DEBUG_STOP_ASSEMBLED). */
int tmpc_debug_set_stop_iteration(tmpc_handle* h, int k);
/* ... and where inside iteration k (tests/test_gpu_step_kernels.py).  Iteration k runs as the solver runs it up to the point, then the call synchronises and returns:
 *   ASSEMBLED    as above (the system unfactored, pass-1 right-hand sides gathered)
 *   AFTER_PASS1  after k_ctrl_b: the predictor's solved W3, TU, Z, dP, dX / dS, Wm, eigmin, c1 / c2 and partial sums stand, P_SIGMU / P_CORR0 are written
 *                (a centering iteration skips pass 1: only k_ctrl_b's back-off test has run)
 *   BEFORE_STEP  pass 2 complete (final direction, Wm, eigmin), k_ctrl_c not run: the iterate has not moved, row k of the trace is not written
 *   AFTER_STEP   after k_ctrl_c, k_update and k_ctrl_d: iteration k is complete, row k of the trace is written */
#define TMPC_DEBUG_STOP_ASSEMBLED 0
#define TMPC_DEBUG_STOP_AFTER_PASS1 1
#define TMPC_DEBUG_STOP_BEFORE_STEP 2
#define TMPC_DEBUG_STOP_AFTER_STEP 3
int tmpc_debug_set_stop_point(tmpc_handle* h, int k, int point);

/* Smallest eigenvalue of nmat symmetric n x n matrices (Householder tridiagonalisation + Sturm multisection). */
int tmpc_debug_min_eig(tmpc_handle* h, int nmat, int n, const double* W, double* out);
/* The same for n <= 8 by the one-thread-per-matrix routine the small shapes use (lane_min_eig8: Householder + Laguerre in registers; round 5). */
int tmpc_debug_min_eig_lane(tmpc_handle* h, int nmat, int n, const double* W, double* out);

/* The step length into the second-order cone (soc_step_eig of csrc/tmpc_t3.h, as k_t3_steps calls it) for nvec pairs (u, du) [nvec][m1], u in the interior of Q^m1:
 * out[i] = -1/theta of the largest theta with u + theta du in Q, or 0 if the ray never leaves the cone.  One wave per pair. */
int tmpc_debug_soc_step(tmpc_handle* h, int nvec, int m1, const double* u, const double* du, double* out);

/* Isolated timing of the block factorisation and of one single-right-hand-side solve on nb copies of one random SPD system:
 * ms_out2[0] = factorisation, [1] = solve (averages over `reps`). */
int tmpc_debug_factor_bench(tmpc_handle* h, int nb, int p, int d, int reps, double* ms_out2);

#ifdef __cplusplus
}
#endif
#endif /* TUNEMPC_HIP_DEBUG_H */
