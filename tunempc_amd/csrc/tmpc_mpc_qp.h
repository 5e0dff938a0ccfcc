// The inequality-constrained tracking-MPC step and its receding-horizon loop (the reference's pmpc.py with h(x, u) >= 0 at every stage, seen through
// closed_loop_tools.check_equivalence and closed_loop_sim): one small structured QP per (problem, initial state),
//   min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j) + 1/2 x_N' Pf_{k_N} x_N,   z_j = [x_j; u_j],   k = k_j = (k0 + j) mod p,
//   s.t. x_{j+1} = A_k x_j + B_k u_j,  x_0 given,   D_k z_j <= d_k (first ndcnt_k rows),   j = 0 .. N-1,
//        and, in the EQ instantiations,   J_k z_j = r_k (first necnt_k rows),  j = 0 .. N-1,   Tx_{k_N} x_N = 0 (nt rows; Tx absent: the identity, x_N = 0),
// solved T times in a row: step t starts at phase (k0 + t) mod p, applies u_0 and moves x <- A_k x + B_k u_0 on the linear plant.  The AFF instantiations
// (below) add the dynamics offset c_k, the terminal cost qf' x_N, the terminal right-hand side t and a plant that is not the model.
// The QUAD instantiations (below) add quadratic slack penalties, the WARM instantiations (below) warm starts between the steps and from a guess.
// Not served: nt > nx; the nonlinear plant is served one launch per step (tunempc_amd.mpc_qp.mpc_closed_loop_plant), not inside the launch.
//
// Method: a primal-dual interior-point method with Mehrotra's predictor-corrector, started infeasible (z = 0 but x_0, s_i = max(d_i, 1), lam_i = 1).  The
// multipliers of the dynamics are not variables: they are the adjoint of the iterate, pi_N = Pf x_N, [pi_j; r_u] = H z_j + q + D' lam_j + [A B]' pi_{j+1}, so
// the dual residual is r_u.  One iteration:
//   pass 1 (backward)   residuals (rows r_in = D z + s - d, dynamics r_dyn = [A B] z_j - x_{j+1}, r_u), then the Newton system, which is the LQ problem with
//                       Hb = H + E' Pi_{j+1} E + D' diag(w) D,  w = lam / (s + rho lam)  (rho = 1e-12, a dual regularisation that bounds w by 1 / rho: its
//                       error in the row equation is rho dlam and vanishes with the step),  h = H z + q + D' (w (r_in + rho lam)) + E' (Pi_{j+1} r_dyn + p_{j+1}):
//                       S = Hb_uu = R' R (Cholesky, in place and together with the right-hand sides: [R | Y | y] = R^-T [S | Hb_ux | h_u]),
//                       Pi_j = Hb_xx - Y' Y,  p_j = h_x - Y' y;
//   sweep (forward)     du = -R^-1 (Y dx + y),  dlam = c - w s + w (r_in + D dz),  ds = -r_in - D dz + rho dlam,  dx+ = E dz + r_dyn, and the step length;
//   corrector           c = (sigma mu - ds_aff dlam_aff) / (s + rho lam), sigma = (mu_aff / mu)^3; by linearity only the change of y is swept backward with
//                       the factors of pass 1 (dh = D' c + E' dp_{j+1}, dy = R^-T dh_u, dp_j = dh_x - Y' dy), then the forward sweep again;
//   step                alpha = min(1, 0.995 alpha_max), one length for primal and dual.
// Stop (tests/mpc_qp_reference.py states the same rule): r_p <= tol, r_d <= tol, mu <= 1e-3 tol max(1, max lam) with
//   r_p = max(max_i |r_in,i| / max(1, |d_i|), max|r_dyn| / max(1, max|x|)),   r_d = max|r_u| / max(1, max_j |H z_j + q + D' lam_j|).
// The factorisation of the pass that meets the stop test is not used: a failed pivot counts only when the test was not met.
//
// Residency: one 256-thread workgroup per instance, fp64 on the vector ALU, the interior-point loop and all T steps in one launch.  The operands of a stage
// ([A B], Pi, Pi E, Hb with the factors, D_k and the vectors of the stage) live in LDS (mpc_qp_lds); A, B, H, D are read again per stage and pass (the ns
// instances of a problem share them in L2).  What an instance keeps per stage for its sweeps -- [Y | R | y], the iterate, the direction, r_in, r_dyn, c --
// lies in a slot of a global workspace (mpc_qp_ws_doubles per slot); the grid is min(instances, MQ_SLOTS) workgroups that loop over the instances.
//
// Order of accumulation: every sum is one thread's sum in ascending order, or a butterfly over the lanes of a wave followed by the four waves in order; nothing
// depends on the slot, on ns or on the other instances.  Control flow is uniform in the workgroup: every decision is taken on block-reduced values or on LDS
// entries that all threads read, there is no exit around a barrier.
//
// Statuses: 0 converged at every step, 1 max_iter reached (an infeasible instance ends here), 2 a stage matrix S not positive definite, 3 non-finite.  An
// instance that fails at step t keeps what it logged before; U, hres from t on, X from t + 1 on and XT are NaN, iters beyond t and nact from t on are -1.
//
// Soft rows (the SOFT instantiation; the reference's preprocessing.add_mpc_slacks, exact L1 penalties): with penalty c_{k,i} < inf row i of stage k reads
//   D_i z - e_i <= d_i,  e_i >= 0,  cost c_i e_i   (penalty = +inf: the hard row above; hard and soft rows mix freely within a stage).
// The slack e and the multiplier nu of e >= 0 are eliminated per row, not lifted into the inputs, so the stage matrices keep their size.  The rules
// (tests/mpc_qp_soft_reference.py states the same ones):
//   start      s = max(d, 1), lam = nu = c / 2, e = s: stationarity in e, c - lam - nu = 0, holds, and both pairs of the row carry the same product; dnu = -dlam and
//              the one step length keep it at every iterate (nu is kept as a variable of its own: c - lam would lose it to cancellation on a violated row);
//   residual   r_in = D z - e + s - d, scaled by max(1, |d|) like a hard row's;
//   weights    from D dz - de + ds - rho dlam = -r_in, s dlam + lam ds = c1 - s lam, -e dlam + nu de = c2 - e nu:  dlam = w (D dz + beta),
//              w = 1 / (s / lam + e / nu + rho),  beta = r_in - s + e + c1 / lam - c2 / nu,  de = -e + c2 / nu + (e / nu) dlam,  ds = -r_in - D dz + de + rho dlam:
//              the Newton system is the same Riccati pass with another weight and right-hand side on that row (h gets D' (lam + w (r_in - s + e)), the
//              corrector column is w (c1 / lam - c2 / nu)); rho has the role it has on a hard row;
//   corrector  c1 = sigma mu - ds_aff dlam_aff,  c2 = sigma mu + de_aff dlam_aff;
//   mu, sigma  every pair counts once: mu = (sum s lam + sum_soft e nu) / (rows + soft rows), mu_aff likewise;
//   step       alpha_max runs over s, lam and, on soft rows, e and nu;
//   stop       unchanged; max lam is taken over lam alone (nu ~ c wherever a row is not violated: a threshold that grew with c would loosen the test).
// hres = max(D z - d) stays and is positive when a soft row of the applied step is violated; nact stays lam > s; nviol counts the rows of stage 0 with e > nu.
// A penalty <= 0 or NaN makes the instance status 3 before its first step.  The LDS vectors e, nu, c lie after MpcQpLds::total (mpc_qp_soft_lds), the
// workspace arrays E, NU, dE, C2 (c2 / nu of the corrector) [N][nd] after mpc_qp_ws_doubles (mpc_qp_soft_ws_doubles).  With SOFT = false the kernel is the
// hard one statement by statement, and a soft launch whose penalties are all +inf takes the hard statements on every row: both give the same bits.
//
// Equality rows and the terminal constraint (the EQ instantiations, with or without SOFT; the reference's pmpc.py carries g(x, u) = 0 at every stage and
// p_operator(x_N - x_ref) = 0 at the end).  An equality row is a hard row WITHOUT a slack (tests/mpc_qp_eq_reference.py states the same rules):
//   multiplier nu: free sign, starts at 0, no step-length limit, no part in mu, sigma or the corrector (the corrector's backward sweep is unchanged);
//   weight     the constant 1 / rho, what an inequality row may reach: Hb gets J' (1 / rho) J, h gets J' (nu + (1 / rho)(J z - r)), the adjoint of the iterate
//              gets J' nu, and the forward sweep gives dnu = (1 / rho)(J dz + J z - r).  The error of the regularisation in the row equation is rho dnu and
//              vanishes with the step; J z - r is taken from the iterate (pass 1), so cancellation at weight 1e12 costs iterations, not accuracy;
//   terminal   the rows enter where the recursion starts: Pi_N = Pf + (1 / rho) Tx' Tx,  p_N = Pf x_N + Tx' (nu_T + (1 / rho) Tx x_N),
//              pi_N = Pf x_N + Tx' nu_T, and after the sweep dnu_T = (1 / rho)(Tx dx_N + Tx x_N).  Tx is read from global memory at these two ends;
//   stop       r_p also takes max_i |J z - r|_i / max(1, |r_i|) and max|Tx x_N| / max(1, max|x|); the scale of r_d takes J' nu into g; max lam stays over lam.
// dnu is needed only for the step, so only the last forward sweep of an iteration computes it (into REQ, whose residual pass 1 writes again).  An instance
// whose rows cannot be met -- N nu too short to reach Tx x_N = 0, a stage-0 row on x_0 alone that x_0 violates -- ends with status 1 like contradictory
// inequality rows.  eres = max|J z_0 - r| of the applied stage (0 at a stage without rows).  LDS: J_k [ne x ld] and the vectors nu, J z - r, r after the hard or
// soft layout (mpc_qp_eq_lds); workspace: NUe, REQ [N][ne] and NUT [nt] after the hard or soft workspace (mpc_qp_eq_ws_doubles); nt <= nx (Tx x_N and dnu_T
// share the last vector slot of the hard layout).  With EQ = false both instantiations are what they were, statement by statement.
//
// The affine problem (the AFF instantiations; they are EQ instantiations, with or without SOFT, and a call without rows runs them with ne = nt = 0):
//   x_{j+1} = A_k x_j + B_k u_j + c_k,   terminal cost 1/2 x_N' Pf x_N + qf_{k_N}' x_N,   Tx_{k_N} x_N = t_{k_N},
// and in the loop the plant x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t (Ap, Bp absent: the model; cp absent: c; W unknown to the controller).  The
// iteration needs no new rule (tests/mpc_qp_affine_reference.py runs the EQ reference on the dense problem with c, t, qf in its vectors):
//   r_dyn = [A B] z_j + c_k - x_{j+1} in pass 1; the start (z = 0 but x_0), the forward sweep and the step rule are unchanged;
//   pi_N = Pf x_N + qf + Tx' nu_T,   p_N = Pf x_N + qf + Tx' (nu_T + (1 / rho)(Tx x_N - t)),   dnu_T = (1 / rho)(Tx dx_N + Tx x_N - t);
//   stop       max|Tx x_N - t| / max(1, max|x|): the scale of today; |c| and |t| enter no scale;
//   plant      A_p, B_p are fetched where E_k is fetched for x <- E [x; u_0], then cp_k + W[b][si][t] is added; hres, eres, nact, nviol stay functions of
//              the applied z_0 of the model's QP.
// c_k, qf, t, cp, W are read from global memory where they are used (as Tx is): no LDS and no workspace of their own, the layouts are those of EQ.  A
// non-finite entry ends the instance with status 3 at the step that meets it (c, qf, t: the stop test of that step; Ap, Bp, cp, W_t: x_{t+1} is
// non-finite and the stop test of step t + 1 sees it); a t that cannot be reached is status 1.  With AFF = false the four instantiations are what they
// were, statement by statement: every statement of AFF stands behind `if (AFF)` or is a value selected by it at compile time.
//
// Quadratic slack penalties (the QUAD instantiations; they are SOFT instantiations: the Zl / Zu of an OCP-QP beside its zl / zu).  penalty2 = Z >= 0 stands
// beside penalty = c; per row of a stage (tests/mpc_qp_quad_reference.py states the same rules):
//   c = inf (Z = 0)   the hard row;      c > 0, Z = 0   the soft row above, its statements and its bits;
//   c > 0, Z > 0      D_i z - e <= d, e >= 0, cost c e + 1/2 Z e^2: two pairs as on a soft row, stationarity in e is c + Z e - lam - nu = 0.
//     start      s = max(d, 1), e = s, lam = nu = (c + Z e) / 2 (both pairs carry the same product; the soft start at Z = 0); dnu = Z de - dlam keeps
//                stationarity at every iterate;
//     weights    with nut = nu + Z e:  w = 1 / (s / lam + e / nut + rho),  beta = r_in - s + c1 / lam + (e nu - c2) / nut,  dlam = w (D dz + beta),
//                de = (c2 - e nu + e dlam) / nut,  ds = -r_in - D dz + de + rho dlam  (h gets D' (lam + w (r_in - s + e nu / nut)), the corrector column is
//                w (c1 / lam - c2 / nut), C2 holds c2 / nut);
//     corrector  c1 = sigma mu - ds_aff dlam_aff,  c2 = sigma mu - de_aff dnu_aff;   the step length runs over s, lam, e, nu with dnu as above;
//                mu, sigma and the stop test as for a soft row;
//   c = 0, Z > 0      pure quadratic: D_i z - e <= d, cost 1/2 Z e^2, ONE pair (no e >= 0 is needed: e = lam / Z >= 0 by itself).  It is a hard row whose
//                dual regularisation is exact instead of vanishing: r_in = D z - lam / Z + s - d,  w = lam / (s + (rho + 1 / Z) lam),
//                ds = -r_in - D dz + (rho + 1 / Z) dlam, the corrector over s + (rho + 1 / Z) lam; start lam = 1; one pair in mu; the reported slack is lam / Z.
// nact stays lam > s; nviol counts the two-pair rows with e > nu and the pure rows with lam > s (on a pure row active means violated); hres is unchanged.
// The row kind is read per row from c and Z in LDS (or from penalty, penalty2 in the loops over the workspace arrays); control flow around barriers stays
// uniform.  Z negative, non-finite or NaN, Z != 0 on a hard row, c negative or NaN, c = 0 with Z = 0: status 3 before the first step.  LDS: the vector Z of
// the stage [nd] after the soft layout (mpc_qp_quad_layout; the EQ part follows it: mpc_qp_quad_eq_layout); the workspace is the soft one (dnu is Z de - dlam of what is stored).
// QUAD is the fourth template parameter of the kernel (mpc_qp_kernel<SOFT, EQ, AFF>() names the six instantiations without it).
// Instantiated twice: <true, false, false, true> for calls without equality, terminal or affine arguments, <true, true, true, true> for the rest (null
// pointers, ne = nt = 0 where there is none).  With QUAD = false the six instantiations are what they were, statement by statement: every statement of QUAD
// stands behind `if (QUAD)` or is a value selected by it at compile time.
//
// Warm starts (the WARM instantiations, one beside each of the eight; WARM is the fifth template parameter).  The reference's Pmpc.step always starts from its
// shifted previous solution; here WARM replaces the start of a step -- the block that fills Z, S, L, E, NU, NUe, NUT -- and nothing else of the iteration.
// The rule (shift by one stage, floors by row kind, fallbacks) is stated at that block and in tests/mpc_qp_warm_reference.py.  In the loop the slot's
// workspace holds the converged iterate of step t - 1 and is shifted in place; at t = 0 the guess arrays are read (MpcQpWarm).  One pass over the stages
// computes D z (and x_N) for the floors with mq_fetch and the LDS slots of the iteration: no LDS and no workspace of its own.  Fallbacks: a guess with a
// non-finite entry starts cold; a warm attempt that ends with status 1 or 2 is solved again from the cold start within the step (iters counts both attempts,
// an infeasible instance costs two runs of max_iter); status 3 is not retried.  The failed attempt stays in the figures of info as well: iters_total and
// iters_max take the sum of both attempts (iters_max may exceed max_iter after a restart), pivmin the smallest pivot of either.  Every decision is taken on
// block-reduced values.  The per-step log
// warmlog [nb][T][ns]: 0 cold, 1 the warm start delivered, 2 the cold restart delivered, -1 from a failed step on.  With WARM = false the eight
// instantiations are what they were, statement by statement: every statement of WARM stands behind `if (WARM)`.
#pragma once
#include "tmpc_closed_loop.h"

namespace tmpc {

constexpr int MQ_INFO = 8;                   // doubles of info per instance (TMPC_MPC_QP_INFO)
constexpr int MQ_SLOTS = 512;                // workgroups (and workspace slots) per launch at the most
constexpr int MQ_NVEC = 24;                  // vector slots of the LDS layout
constexpr double MQ_RHO = 1e-12, MQ_STEP_BACK = 0.995, MQ_MU_FACTOR = 1e-3;
constexpr double MQ_RINV = 1.0 / MQ_RHO;     // the weight of an equality row
enum { MQ_OK = 0, MQ_MAXITER = 1, MQ_NOT_CONVEX = 2, MQ_NONFINITE = 3 };

struct MpcQpLds { int ld, ldp, lv, oE, oP, oW, oH, oD, oV, oR, total; };      // offsets in doubles
__host__ __device__ inline MpcQpLds mpc_qp_lds(int nx, int mb, int nd) {
  MpcQpLds l;
  const int n = nx + mb;
  l.ld = (n + 1) | 1; l.ldp = nx | 1;
  l.lv = n + 1 > nd ? n + 1 : nd;
  l.oE = 0;                                  // E_k = [A_k B_k] [nx x n]
  l.oP = l.oE + nx * l.ld;                   // Pi_{j+1}, then Pi_j [nx x nx]
  l.oW = l.oP + nx * l.ldp;                  // Pi E [nx x n]
  l.oH = l.oW + nx * l.ld;                   // H_k, then Hb, then [Y | R | y] in its rows nx .. n-1 (column n: h_u) [n x (n + 1)]
  l.oD = l.oH + n * l.ld;                    // D_k [nd x n]
  l.oV = l.oD + nd * l.ld;                   // MQ_NVEC vectors of lv doubles
  l.oR = l.oV + MQ_NVEC * l.lv;              // block reductions [8]
  const long long total = (long long)l.oR + 8;
  l.total = total > 0x7fffffffLL / 8 ? 0x7fffffff / 8 : (int)total;
  return l;
}

// doubles of workspace per slot: Z, dZ [(N+1)][n]; S, L, dS, dL, RIN, COR [N][nd]; RDYN [N][nx]; FAC [N][mb][n + 1]
__host__ __device__ inline long long mpc_qp_ws_doubles(int nx, int mb, int nd, int N) {
  const long long n = nx + mb;
  return 2LL * (N + 1) * n + 6LL * N * nd + (long long)N * nx + (long long)N * mb * (n + 1);
}

// The SOFT instantiation: the hard layout, then the vectors e, nu, c of the stage [nd] each; the hard workspace, then E, NU, dE, C2 [N][nd] each.
struct MpcQpSoftLds { MpcQpLds h; int oEs, oNu, oC, total; };
__host__ __device__ inline MpcQpSoftLds mpc_qp_soft_lds(int nx, int mb, int nd) {
  MpcQpSoftLds l;
  l.h = mpc_qp_lds(nx, mb, nd);
  l.oEs = l.h.total; l.oNu = l.oEs + nd; l.oC = l.oNu + nd;
  const long long total = (long long)l.oC + nd;
  l.total = total > 0x7fffffffLL / 8 ? 0x7fffffff / 8 : (int)total;
  return l;
}
__host__ __device__ inline long long mpc_qp_soft_ws_doubles(int nx, int mb, int nd, int N) {
  return mpc_qp_ws_doubles(nx, mb, nd, N) + 4LL * N * nd;
}

// The QUAD instantiations: the soft layout, then the vector Z of the stage [nd]; the soft workspace (the rules need no array of their own).
struct MpcQpQuadLds { MpcQpSoftLds s; int oZ, total; };
__host__ __device__ inline MpcQpQuadLds mpc_qp_quad_layout(int nx, int mb, int nd) {
  MpcQpQuadLds l;
  l.s = mpc_qp_soft_lds(nx, mb, nd);
  l.oZ = l.s.total;
  const long long total = (long long)l.oZ + nd;
  l.total = total > 0x7fffffffLL / 8 ? 0x7fffffff / 8 : (int)total;
  return l;
}

// The EQ instantiations: the hard (or soft) layout, then J_k [ne x ld] and the vectors nu, J z - r, r of the stage [ne] each; the hard (or soft) workspace,
// then NUe, REQ [N][ne] each and NUT [nt].
struct MpcQpEqLds { int base, oJ, oNu, oReq, oR, total; };
__host__ __device__ inline MpcQpEqLds mpc_qp_eq_lds(int nx, int mb, int nd, int ne, bool soft) {
  MpcQpEqLds l;
  l.base = soft ? mpc_qp_soft_lds(nx, mb, nd).total : mpc_qp_lds(nx, mb, nd).total;
  const long long ld = ((nx + mb + 1) | 1);
  const long long oNu = (long long)l.base + (long long)ne * ld, total = oNu + 3LL * ne;
  const bool big = total > 0x7fffffffLL / 8;
  l.oJ = l.base; l.oNu = big ? l.base : (int)oNu; l.oReq = l.oNu + (big ? 0 : ne); l.oR = l.oReq + (big ? 0 : ne);
  l.total = big ? 0x7fffffff / 8 : (int)total;
  return l;
}
__host__ __device__ inline long long mpc_qp_eq_ws_doubles(int nx, int mb, int nd, int N, int ne, int nt, bool soft) {
  return (soft ? mpc_qp_soft_ws_doubles(nx, mb, nd, N) : mpc_qp_ws_doubles(nx, mb, nd, N)) + 2LL * N * ne + nt;
}

// The QUAD instantiation with EQ: the soft EQ layout moved behind Z (nd doubles further); the workspace is that of the soft EQ kernel.
__host__ __device__ inline MpcQpEqLds mpc_qp_quad_eq_layout(int nx, int mb, int nd, int ne) {
  MpcQpEqLds l = mpc_qp_eq_lds(nx, mb, nd, ne, true);
  if (l.total < 0x7fffffff / 8 && (long long)l.total + nd <= 0x7fffffffLL / 8) { l.base += nd; l.oJ += nd; l.oNu += nd; l.oReq += nd; l.oR += nd; l.total += nd; }
  else l.total = 0x7fffffff / 8;
  return l;
}

// The arguments of the AFF instantiations, each or null: c [nb][p][nx], qf [nb][p][nx], t [nb][p][nt], Ap [nb][p][nx][nx] and Bp [nb][p][nx][mb] (both or
// neither), cp [nb][p][nx] (null: c), W [nb][ns][T][nx].
struct MpcQpAff { const double* c; const double* qf; const double* t; const double* Ap; const double* Bp; const double* cp; const double* W; };

// The arguments of the WARM instantiations.  flags: bit 0 every step t > 0 of the loop starts from the shifted iterate of step t - 1, bit 1 step 0 starts
// from the guess, bit 2 the guess is shifted by one stage first.  floor: delta of the floors.  The guess, each or null (null: zeros): X [nb][ns][N+1][nx],
// U [nb][ns][N][mb], Lam, Eps [nb][ns][N][nd], Nu [nb][ns][N][ne], NuT [nb][ns][nt] (what an earlier call returned as Xol, Uol, Lam, Eol, Nu, NuT).
// log int [nb][T][ns] or null: 0 cold, 1 the warm start delivered the step, 2 the warm attempt failed and the cold restart delivered, -1 from a failed step on.
struct MpcQpWarm { int flags; double floor; const double* X; const double* U; const double* Lam; const double* Eps; const double* Nu; const double* NuT; int* log; };

// (QUAD) Opens every block of statements that only a row with Z > 0 takes.  The compiler may not move an empty volatile statement, so such a block stays a
// block of its own: it is not merged into the soft row's statements beside it, which are then compiled as they are in the SOFT instantiation -- what the
// promise "a row with Z = 0 gives the bits of the soft kernel" rests on (products and sums are fused within a block).
#define MQ_QUAD_BLOCK asm volatile("")

__device__ __forceinline__ double mq_dot(const double* __restrict__ a, const double* __restrict__ b, int len) {
  double acc = 0.0;
  for (int c = 0; c < len; ++c) acc = fma(a[c], b[c], acc);
  return acc;
}

// op 0: sum, 1: max, 2: min over the workgroup; every thread returns the same value.  Butterfly over the lanes, then the four waves in order.
template <int OP> __device__ __forceinline__ double mq_block(double v, double* red, int tid) {
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o, 64);
    v = OP == 0 ? v + u : (OP == 1 ? fmax(v, u) : fmin(v, u));
  }
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double a = red[0], b = red[1], c = red[2], d = red[3];
  const double r = OP == 0 ? ((a + b) + c) + d : (OP == 1 ? fmax(fmax(a, b), fmax(c, d)) : fmin(fmin(a, b), fmin(c, d)));
  __syncthreads();
  return r;
}

// E_k, D_k (m rows) and optionally H_k (symmetrised) of stage k into LDS; tx < cw columns, ty first row, rs row stride.
__device__ __forceinline__ void mq_fetch(double* El, double* Hl, double* Dl, int ld, const double* __restrict__ Ak, const double* __restrict__ Bk,
                                         const double* __restrict__ Hk, const double* __restrict__ Dk, int nx, int mb, int m, int tx, int ty, int rs) {
  const int n = nx + mb;
  if (tx < n) {
    for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
    if (Hk) for (int r = ty; r < n; r += rs) Hl[r * ld + tx] = 0.5 * (Hk[r * n + tx] + Hk[tx * n + r]);
    for (int i = ty; i < m; i += rs) Dl[i * ld + tx] = Dk[i * n + tx];
  }
}

// grid: min(nb * ns, MQ_SLOTS) workgroups; instance = b * ns + s.  cw = 1 << lcw: power of two >= n (<= 64).  A [nb][p][nx][nx], B [nb][p][nx][mb],
// H [nb][p][n][n], q [nb][p][n] or null, Pf [nb][p][nx][nx] or null, D [nb][p][nd][n] and d [nb][p][nd] (null when nd = 0), ndcnt [nb][p] or null (all nd rows;
// counts are clamped to 0 .. nd), X0 [nb][ns][nx]; ws: gridDim.x slots of mpc_qp_ws_doubles.  Outputs: U0 [nb][ns][mb], XT [nb][ns][nx], info [nb][ns][8];
// each or null: X [nb][T+1][ns][nx], U [nb][T][ns][mb], iters, nact int [nb][T][ns], hres [nb][T][ns], Xol [nb][ns][N+1][nx], Uol [nb][ns][N][mb],
// Lam [nb][ns][N][nd] (the open-loop solution of step 0).  SOFT: penalty [nb][p][nd] (+inf: hard row), and each or null Eol [nb][ns][N][nd], nviol int
// [nb][T][ns]; ws: gridDim.x slots of mpc_qp_soft_ws_doubles, LDS of mpc_qp_soft_lds.  Without SOFT the three are not read or written.
// EQ: J [nb][p][ne][n] (null when ne = 0), req [nb][p][ne] or null (zero), necnt [nb][p] or null (all ne rows; clamped to 0 .. ne), Tx [nb][p][nt][nx] or null
// (nt = nx: the identity), nt <= nx, and each or null Nu [nb][ns][N][ne], NuT [nb][ns][nt], eres [nb][T][ns]; ws: slots of mpc_qp_eq_ws_doubles, LDS of
// mpc_qp_eq_lds.  Without EQ none of these is read or written.  AFF: aff (MpcQpAff above); without AFF it is not read.
// QUAD: pen2g [nb][p][nd] (penalty2 beside penalty); without QUAD it is not read.  WARM: wm (MpcQpWarm above); without WARM it is not read.
// (WARM) the second launch bound, waves per SIMD the compiler has to leave room for: 0 (no bound: the other fifteen instantiations carry no attribute for
// it, as before) but for the WARM instantiation of the plain soft kernel, whose cold twin runs two waves per SIMD at 246 registers: its few registers over 256 go to scratch instead of halving the occupancy.
#define MQ_WAVES(SOFT, EQ, QUAD, WARM) (((WARM) && (SOFT) && !(EQ) && !(QUAD)) ? 2 : 0)
template <bool SOFT, bool EQ, bool AFF, bool QUAD, bool WARM = false>
__global__ void __launch_bounds__(LQR_NT, MQ_WAVES(SOFT, EQ, QUAD, WARM)) k_mpc_qp(int p, int nx, int mb, int nd, int lcw, int N, int ns, int T, int k0, long long ninst,
                                                   const double* __restrict__ Ag, const double* __restrict__ Bg, const double* __restrict__ Hg,
                                                   const double* __restrict__ qg, const double* __restrict__ Pfg, const double* __restrict__ Dg,
                                                   const int* __restrict__ ndcntg, const double* __restrict__ dg, const double* __restrict__ X0g, double tol,
                                                   int max_iter, double* wsg, double* __restrict__ U0g, double* __restrict__ XTg, double* __restrict__ infog,
                                                   double* __restrict__ Xg, double* __restrict__ Ug, int* __restrict__ itersg, int* __restrict__ nactg,
                                                   double* __restrict__ hresg, double* __restrict__ Xolg, double* __restrict__ Uolg,
                                                   double* __restrict__ Lamg, const double* __restrict__ peng, double* __restrict__ Eolg,
                                                   int* __restrict__ nviolg, int ne, const double* __restrict__ Jg, const double* __restrict__ reqg,
                                                   const int* __restrict__ necntg, int nt, const double* __restrict__ Txg, double* __restrict__ Nug,
                                                   double* __restrict__ NuTg, double* __restrict__ eresg, MpcQpAff aff, const double* __restrict__ pen2g,
                                                   MpcQpWarm wm) {
  static_assert(EQ || !AFF, "the AFF instantiations are EQ instantiations");
  static_assert(SOFT || !QUAD, "the QUAD instantiations are SOFT instantiations");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const MpcQpLds Ly = mpc_qp_lds(nx, mb, nd);
  const int ld = Ly.ld, ldp = Ly.ldp, lv = Ly.lv;
  double* El = lds + Ly.oE; double* Pl = lds + Ly.oP; double* Wl = lds + Ly.oW; double* Hl = lds + Ly.oH; double* Dl = lds + Ly.oD; double* red = lds + Ly.oR;
  double* V = lds + Ly.oV;
  double* zv = V; double* xn = V + lv; double* lamv = V + 2 * lv; double* sv = V + 3 * lv; double* ddv = V + 4 * lv; double* wv_ = V + 5 * lv;
  double* rinv = V + 6 * lv; double* bsv = V + 7 * lv; double* gq = V + 8 * lv; double* fullv = V + 9 * lv; double* hp = V + 10 * lv; double* rdynv = V + 11 * lv;
  double* vv = V + 12 * lv; double* pin = V + 13 * lv; double* pv = V + 14 * lv; double* dxa = V + 15 * lv; double* dxb = V + 16 * lv; double* dzv = V + 17 * lv;
  double* corv = V + 18 * lv; double* xcur = V + 19 * lv; double* dgv = V + 20 * lv; double* dyv = V + 21 * lv; double* qv = V + 22 * lv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const long long wsn = EQ ? mpc_qp_eq_ws_doubles(nx, mb, nd, N, ne, nt, SOFT) : (SOFT ? mpc_qp_soft_ws_doubles(nx, mb, nd, N) : mpc_qp_ws_doubles(nx, mb, nd, N));
  double* ws = wsg + (size_t)blockIdx.x * wsn;
  double* Z = ws; double* dZ = Z + (size_t)(N + 1) * n; double* Sg = dZ + (size_t)(N + 1) * n; double* Lg = Sg + (size_t)N * nd; double* dSg = Lg + (size_t)N * nd;
  double* dLg = dSg + (size_t)N * nd; double* RIN = dLg + (size_t)N * nd; double* COR = RIN + (size_t)N * nd; double* RDYN = COR + (size_t)N * nd;
  double* FAC = RDYN + (size_t)N * nx;
  const int fs = mb * (n + 1);                                               // doubles of [Y | R | y] per stage
  double* Eg = FAC + (size_t)N * fs; double* NUg = Eg + (size_t)N * nd; double* dEg = NUg + (size_t)N * nd; double* C2g = dEg + (size_t)N * nd;   // (SOFT only)
  double* ev = lds + Ly.total; double* nuv = ev + nd; double* cv = nuv + nd;                                                                   // (SOFT only)
  double* zqv = cv + nd;                                                     // (QUAD only) Z of the stage
  // (EQ only) J_k and the vectors nu, J z - r, r (then nu + (1 / rho)(J z - r)) of the stage; Tx x_N, then dnu_T; the multipliers and the residuals per stage
  double* Jl = lds + (SOFT ? Ly.total + 3 * nd : Ly.total); double* nuev = Jl + ne * ld; double* reqv = nuev + ne; double* rrv = reqv + ne;
  if (QUAD) { Jl += nd; nuev += nd; reqv += nd; rrv += nd; }                 // (QUAD) the EQ part follows Z: mpc_qp_quad_eq_layout
  double* tv = V + 23 * lv;
  double* NUe = ws + (SOFT ? mpc_qp_soft_ws_doubles(nx, mb, nd, N) : mpc_qp_ws_doubles(nx, mb, nd, N)); double* REQ = NUe + (size_t)N * ne;
  double* NUT = REQ + (size_t)N * ne;

  for (long long inst = blockIdx.x; inst < ninst; inst += gridDim.x) {
    const size_t b = (size_t)(inst / ns), si = (size_t)(inst % ns);
    const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* H = Hg + b * p * n * n;
    const double* q = qg ? qg + b * p * n : nullptr; const double* Pf = Pfg ? Pfg + b * p * nx * nx : nullptr;
    const double* D = nd > 0 ? Dg + b * p * nd * n : nullptr; const double* dd = nd > 0 ? dg + b * p * nd : nullptr;
    const int* ndcnt = ndcntg ? ndcntg + b * p : nullptr;
    auto rows_of = [&](int k) { return nd > 0 ? (ndcnt ? max(0, min(nd, ndcnt[k])) : nd) : 0; };
    const double* pen = SOFT ? peng + b * p * nd : nullptr;
    const double* pen2 = QUAD ? pen2g + b * p * nd : nullptr;
    const double* J = EQ && ne > 0 ? Jg + b * p * ne * n : nullptr; const double* rq = EQ && reqg ? reqg + b * p * ne : nullptr;
    const int* necnt = EQ && necntg ? necntg + b * p : nullptr;
    const double* Tx = EQ && Txg ? Txg + b * p * nt * nx : nullptr;
    auto erows_of = [&](int k) { return ne > 0 ? (necnt ? max(0, min(ne, necnt[k])) : ne) : 0; };
    // (AFF) the offsets of the model and of the plant, the terminal vectors, the plant's matrices (absent: the model's) and the disturbance of this instance
    const double* cof = AFF && aff.c ? aff.c + b * p * nx : nullptr; const double* qfv = AFF && aff.qf ? aff.qf + b * p * nx : nullptr;
    const double* trh = AFF && aff.t ? aff.t + b * p * nt : nullptr;
    const double* Ap = AFF && aff.Ap ? aff.Ap + b * p * nx * nx : A; const double* Bp = AFF && aff.Bp ? aff.Bp + b * p * nx * mb : B;
    const double* cpl = AFF ? (aff.cp ? aff.cp + b * p * nx : cof) : nullptr;
    const double* Wd = AFF && aff.W ? aff.W + (b * ns + si) * T * nx : nullptr;

    if (tid < nx) {
      const double v = X0g[(b * ns + si) * nx + tid];
      xcur[tid] = v;
      if (Xg) Xg[((b * (T + 1)) * ns + si) * nx + tid] = v;
    }
    __syncthreads();
    int status = MQ_OK, done = 0, it_total = 0, it_max = 0;
    double mu = 0.0, rp = 0.0, rd = 0.0, pivmin = INFINITY;
    if (SOFT) {                                                              // a penalty <= 0 or NaN: the instance ends before its first step
      double bad = 0.0;
      if (!QUAD) for (int e = tid; e < p * nd; e += LQR_NT) if (!(pen[e] > 0.0)) bad = 1.0;
      if (QUAD) for (int e = tid; e < p * nd; e += LQR_NT) {                 // Z >= 0 and finite, 0 on a hard row; c > 0, or c = 0 with Z > 0
        const double c = pen[e], z = pen2[e];
        if (!(z >= 0.0 && z < INFINITY) || !(c > 0.0 || (c == 0.0 && z > 0.0)) || (c == INFINITY && z != 0.0)) bad = 1.0;
      }
      if (mq_block<1>(bad, red, tid) > 0.0) status = MQ_NONFINITE;
    }

    for (int t = 0; t < T; ++t) {
      const int k0s = (k0 + t % p) % p;
      int its = 0, nact = -1, nviol = -1;
      double hres = qnan, eres = qnan;
      int wcode = -1;                                                        // (WARM) the step's entry of the log
      if (status == MQ_OK) {                                                 // (uniform: status is the same in every thread)
        // ---- start of the step: z = 0 but x_0, s = max(d, 1), lam = 1, no direction
        int mt = 0;
        for (int j = 0; j < N; ++j) mt += rows_of((k0s + j % p) % p);
        // (SOFT) soft_at(e): entry e = j nd + i of the [N][nd] arrays is a soft row of this step
        auto soft_at = [&](int e) {
          const int j = e / nd, i = e - j * nd, k = (k0s + j % p) % p;
          if (QUAD) return i < rows_of(k) && pen[k * nd + i] < INFINITY && pen[k * nd + i] > 0.0;      // (a pure quadratic row, c = 0, has one pair)
          return i < rows_of(k) && pen[k * nd + i] < INFINITY;
        };
        // (QUAD) zq_at(e): Z of entry e, pure_at(e): entry e is a pure quadratic row (c = 0: one pair, soft_at is false)
        auto zq_at = [&](int e) { const int j = e / nd, i = e - j * nd, k = (k0s + j % p) % p; return pen2[k * nd + i]; };
        auto pure_at = [&](int e) { const int j = e / nd, i = e - j * nd, k = (k0s + j % p) % p; return i < rows_of(k) && pen[k * nd + i] == 0.0; };
        // (WARM) warm_now: this attempt starts warm (block-uniform).  In the loop the slot holds the converged iterate of step t - 1; at t = 0 the guess is
        // taken when every entry of it is finite (a failed predecessor returns NaN).  its_warm: the iterations of a warm attempt that failed.
        bool warm_now = false, retried = false;
        int its_warm = 0;
        if (WARM) {
          warm_now = t > 0 ? (wm.flags & 1) != 0 : (wm.flags & 2) != 0;
          if (t == 0 && warm_now) {
            const size_t gi = b * ns + si;
            auto fin = [](double v) { return fabs(v) < INFINITY; };
            double bad = 0.0;
            for (int e = tid; e < (N + 1) * nx; e += LQR_NT) if (!fin(wm.X[gi * (N + 1) * nx + e])) bad = 1.0;
            for (int e = tid; e < N * mb; e += LQR_NT) if (!fin(wm.U[gi * N * mb + e])) bad = 1.0;
            if (wm.Lam) for (int e = tid; e < N * nd; e += LQR_NT) if (!fin(wm.Lam[gi * N * nd + e])) bad = 1.0;
            if (SOFT) if (wm.Eps) for (int e = tid; e < N * nd; e += LQR_NT) if (!fin(wm.Eps[gi * N * nd + e])) bad = 1.0;
            if (EQ) {
              if (wm.Nu) for (int e = tid; e < N * ne; e += LQR_NT) if (!fin(wm.Nu[gi * N * ne + e])) bad = 1.0;
              if (wm.NuT) if (tid < nt) if (!fin(wm.NuT[gi * nt + tid])) bad = 1.0;
            }
            if (mq_block<1>(bad, red, tid) > 0.0) warm_now = false;
          }
        }
      mq_start:                                                              // (WARM) the cold restart of a failed warm attempt comes back here
        if (WARM && warm_now) {
          // ---- (WARM) start of the step from the previous iterate (tests/mpc_qp_warm_reference.py states the same rule; delta = wm.floor):
          //   shift    new stage j takes old stage j + 1 for j <= N - 2 (same phase, same rows), x_0 is the measured state, u_{N-1} repeats the old last input,
          //            x_N = A_k x_{N-1} + B_k u_{N-1} (+ c_k) at the phase of the new last stage; lam, e and the equality multipliers shift the same way and
          //            are zero at the new last stage before the floors; nu_T is kept.  Without a shift (a guess for the same phase) only x_0 is replaced;
          //   floors   hard row  s = max(d - D z, delta), lam = max(lam, delta);   L1 and L1 + L2 rows  e = max(e, delta), lam = clip(lam, delta,
          //            c + Z e - delta), nu = c + Z e - lam (the invariant c + Z e - lam - nu = 0 holds exactly), lam = nu = (c + Z e) / 2 when
          //            c + Z e < 2 delta, s = max(d - D z + e, delta);   pure quadratic row  lam = max(lam, delta), s = max(d - D z + lam / Z, delta);
          //            equality and terminal multipliers free; every direction zero.  s and nu of the previous iterate are not read.
          const bool shifted = t > 0 || (wm.flags & 4) != 0;
          if (t == 0) {                                                      // the guess into the slot as it is given
            const size_t gi = b * ns + si;
            for (int e = tid; e < (N + 1) * n; e += LQR_NT) {
              const int j = e / n, c = e - j * n;
              Z[e] = c < nx ? wm.X[(gi * (N + 1) + j) * nx + c] : (j < N ? wm.U[(gi * N + j) * mb + c - nx] : 0.0);
            }
            for (int e = tid; e < N * nd; e += LQR_NT) {
              Lg[e] = wm.Lam ? wm.Lam[gi * N * nd + e] : 0.0;
              if (SOFT) Eg[e] = wm.Eps ? wm.Eps[gi * N * nd + e] : 0.0;
            }
            if (EQ) {
              for (int e = tid; e < N * ne; e += LQR_NT) NUe[e] = wm.Nu ? wm.Nu[gi * N * ne + e] : 0.0;
              if (tid < nt) NUT[tid] = wm.NuT ? wm.NuT[gi * nt + tid] : 0.0;
            }
            __syncthreads();
          }
          if (shifted) {                                                     // in place: a thread owns a column of an array and walks the stages upward
            for (int c = tid; c < n; c += LQR_NT) {
              for (int j = 0; j + 1 < N; ++j) Z[(size_t)j * n + c] = Z[(size_t)(j + 1) * n + c];
              if (c < nx) Z[(size_t)(N - 1) * n + c] = Z[(size_t)N * n + c];
            }
            for (int c = tid; c < nd; c += LQR_NT) {
              for (int j = 0; j + 1 < N; ++j) {
                Lg[(size_t)j * nd + c] = Lg[(size_t)(j + 1) * nd + c];
                if (SOFT) Eg[(size_t)j * nd + c] = Eg[(size_t)(j + 1) * nd + c];
              }
              Lg[(size_t)(N - 1) * nd + c] = 0.0;
              if (SOFT) Eg[(size_t)(N - 1) * nd + c] = 0.0;
            }
            if (EQ) for (int c = tid; c < ne; c += LQR_NT) {
              for (int j = 0; j + 1 < N; ++j) NUe[(size_t)j * ne + c] = NUe[(size_t)(j + 1) * ne + c];
              NUe[(size_t)(N - 1) * ne + c] = 0.0;
            }
            __syncthreads();
          }
          if (tid < nx) Z[tid] = xcur[tid];
          for (int e = tid; e < (N + 1) * n; e += LQR_NT) dZ[e] = 0.0;
          if (EQ) for (int e = tid; e < N * ne; e += LQR_NT) REQ[e] = 0.0;
          __syncthreads();
          for (int j = 0; j < N; ++j) {                                      // one pass over the stages: D z for the floors, x_N at the last stage
            const int k = (k0s + j % p) % p, m = rows_of(k);
            mq_fetch(El, nullptr, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, nullptr, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
            if (tid < n) zv[tid] = Z[(size_t)j * n + tid];
            __syncthreads();
            for (int i = tid; i < nd; i += LQR_NT) {
              const size_t e = (size_t)j * nd + i;
              double s = 1.0, lam = 0.0, ee = 0.0, nu = 0.0;                 // an absent row: the values of the cold start
              if (i < m) {
                const double fl = wm.floor, slack = dd[k * nd + i] - mq_dot(Dl + i * ld, zv, n);
                const double c = SOFT ? pen[k * nd + i] : INFINITY, zq = QUAD ? pen2[k * nd + i] : 0.0;
                lam = Lg[e];
                if (c < INFINITY && (!QUAD || c > 0.0)) {                    // two pairs
                  ee = fmax(Eg[e], fl);
                  const double tot = c + zq * ee;
                  lam = tot < 2.0 * fl ? 0.5 * tot : fmin(fmax(lam, fl), tot - fl);
                  nu = tot - lam;
                  s = fmax(slack + ee, fl);
                } else if (QUAD && c == 0.0) {                               // pure quadratic
                  lam = fmax(lam, fl);
                  s = fmax(slack + lam * (1.0 / zq), fl);
                } else {
                  lam = fmax(lam, fl);
                  s = fmax(slack, fl);
                }
              }
              Sg[e] = s; Lg[e] = lam; dSg[e] = 0.0; dLg[e] = 0.0; RIN[e] = 0.0; COR[e] = 0.0;
              if (SOFT) { Eg[e] = ee; NUg[e] = nu; dEg[e] = 0.0; C2g[e] = 0.0; }
            }
            if (shifted && j == N - 1 && tid < nx) {
              double v = mq_dot(El + tid * ld, zv, n);
              if (AFF) if (cof) v += cof[k * nx + tid];
              Z[(size_t)N * n + tid] = v;
            }
            __syncthreads();
          }
        } else {                                                             // the cold start, its statements where they were (not indented)
        for (int e = tid; e < (N + 1) * n; e += LQR_NT) { Z[e] = e < nx ? xcur[e] : 0.0; dZ[e] = 0.0; }
        for (int e = tid; e < N * nd; e += LQR_NT) {
          const int j = e / nd, i = e - j * nd, k = (k0s + j % p) % p;
          const bool on = i < rows_of(k);
          Sg[e] = on ? fmax(dd[k * nd + i], 1.0) : 1.0; Lg[e] = on ? 1.0 : 0.0;
          dSg[e] = 0.0; dLg[e] = 0.0; RIN[e] = 0.0; COR[e] = 0.0;
          if (SOFT) {                                                        // lam = nu = c / 2, e = s; zero on hard and absent rows
            bool sf = on && pen[k * nd + i] < INFINITY;
            if (QUAD) sf = sf && pen[k * nd + i] > 0.0;
            double hc = sf ? 0.5 * pen[k * nd + i] : 0.0;
            if (QUAD) if (sf && pen2[k * nd + i] > 0.0) { MQ_QUAD_BLOCK; hc = 0.5 * (pen[k * nd + i] + pen2[k * nd + i] * Sg[e]); }      // lam = nu = (c + Z e) / 2, e = s
            if (sf) Lg[e] = hc;
            NUg[e] = hc; Eg[e] = sf ? Sg[e] : 0.0; dEg[e] = 0.0; C2g[e] = 0.0;
          }
        }
        if (EQ) {                                                            // nu = 0
          for (int e = tid; e < N * ne; e += LQR_NT) { NUe[e] = 0.0; REQ[e] = 0.0; }
          if (tid < nt) NUT[tid] = 0.0;
        }
        }                                                                    // (WARM) end of the cold start
        int mp = mt;                                                         // complementarity pairs: one per row, one more per soft row
        if (SOFT) {
          double cnt = 0.0;
          for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) cnt += 1.0;
          mp = mt + (int)mq_block<0>(cnt, red, tid);
        }
        __syncthreads();
        const int kN = (k0s + N % p) % p;
        auto tx_at = [&](int i, int c) { return Tx ? Tx[((size_t)kN * nt + i) * nx + c] : (i == c ? 1.0 : 0.0); };      // (EQ) row i of Tx_{k_N}

        for (int it = 0;; ++it) {
          its = it;
          // ================================================================ pass 1: residuals and factorisation, j = N-1 .. 0
          if (tx < nx) for (int r = ty; r < nx; r += rs) Pl[r * ldp + tx] = Pf ? 0.5 * (Pf[((size_t)kN * nx + r) * nx + tx] + Pf[((size_t)kN * nx + tx) * nx + r]) : 0.0;
          if (tid < nx) xn[tid] = Z[(size_t)N * n + tid];
          __syncthreads();
          double a_rp = 0.0, a_dyn = 0.0, a_x = 0.0, a_rd = 0.0, a_g = 0.0, a_lam = 0.0;
          if (tid < nx) {
            double v = mq_dot(Pl + tid * ldp, xn, nx);
            if (AFF) if (qfv) v += qfv[kN * nx + tid];
            pin[tid] = v; pv[tid] = v;
            a_x = cl_absmax(a_x, xn[tid]);
          }
          int facfail = 0;
          __syncthreads();
          if (EQ) {                                                          // the terminal rows: Tx x_N, pi_N, p_N and Pi_N
            if (tid < nt) {
              double acc = 0.0;
              for (int c = 0; c < nx; ++c) acc = fma(tx_at(tid, c), xn[c], acc);
              if (AFF) if (trh) acc -= trh[kN * nt + tid];
              tv[tid] = acc;
            }
            __syncthreads();
            if (tid < nx) {
              double s1 = 0.0, s2 = 0.0;
              for (int i = 0; i < nt; ++i) { const double x = tx_at(i, tid), nuT = NUT[i]; s1 = fma(x, nuT, s1); s2 = fma(x, nuT + MQ_RINV * tv[i], s2); }
              pin[tid] += s1; pv[tid] += s2;
            }
            if (tx < nx) for (int r = ty; r < nx; r += rs) {
              double acc = 0.0;
              for (int i = 0; i < nt; ++i) acc = fma(tx_at(i, r) * MQ_RINV, tx_at(i, tx), acc);
              Pl[r * ldp + tx] += acc;
            }
            __syncthreads();
          }
          for (int j = N - 1; j >= 0; --j) {
            const int k = (k0s + j % p) % p, m = rows_of(k);
            mq_fetch(El, Hl, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, H + (size_t)k * n * n, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
            if (tid < n) { zv[tid] = Z[(size_t)j * n + tid]; qv[tid] = q ? q[k * n + tid] : 0.0; }
            if (tid >= 64 && tid < 64 + nx) xn[tid - 64] = Z[(size_t)(j + 1) * n + tid - 64];
            for (int i = tid; i < m; i += LQR_NT) { lamv[i] = Lg[(size_t)j * nd + i]; sv[i] = Sg[(size_t)j * nd + i]; ddv[i] = dd[k * nd + i]; }
            if (SOFT) for (int i = tid; i < m; i += LQR_NT) { ev[i] = Eg[(size_t)j * nd + i]; nuv[i] = NUg[(size_t)j * nd + i]; cv[i] = pen[k * nd + i]; }
            if (QUAD) for (int i = tid; i < m; i += LQR_NT) zqv[i] = pen2[k * nd + i];
            const int me = EQ ? erows_of(k) : 0;
            if (EQ) {
              if (tx < n) for (int i = ty; i < me; i += rs) Jl[i * ld + tx] = J[((size_t)k * ne + i) * n + tx];
              for (int i = tid; i < me; i += LQR_NT) { nuev[i] = NUe[(size_t)j * ne + i]; rrv[i] = rq ? rq[k * ne + i] : 0.0; }
            }
            __syncthreads();
            // ---- A: the residuals of the rows and of the dynamics, H z + q, Pi E
            for (int e = tid; e < m + nx + n; e += LQR_NT) {
              if (e < m) {
                const double lam = lamv[e], s = sv[e];
                double r = mq_dot(Dl + e * ld, zv, n) + s - ddv[e];
                double w = lam / (s + MQ_RHO * lam);
                double bs = w * (r + MQ_RHO * lam);
                if (SOFT) if (cv[e] < INFINITY) if (!QUAD || cv[e] > 0.0) {  // lam + w beta of the predictor, beta = r_in - s + e
                  const double ee = ev[e];
                  r = mq_dot(Dl + e * ld, zv, n) - ee + s - ddv[e];
                  w = 1.0 / (s / lam + ee / nuv[e] + MQ_RHO);
                  bs = lam + w * (r - s + ee);
                }
                if (QUAD) if (cv[e] < INFINITY && cv[e] > 0.0 && zqv[e] > 0.0) {      // L1 + L2: nut = nu + Z e, beta = r_in - s + e nu / nut
                  MQ_QUAD_BLOCK;
                  const double ee = ev[e], nut = nuv[e] + zqv[e] * ee;
                  w = 1.0 / (s / lam + ee / nut + MQ_RHO);
                  bs = lam + w * (r - s + ee * nuv[e] / nut);
                }
                if (QUAD) if (cv[e] == 0.0) {                                // pure quadratic: the hard row with rho + 1 / Z, r_in = D z - lam / Z + s - d
                  MQ_QUAD_BLOCK;
                  const double zi = 1.0 / zqv[e], rz = MQ_RHO + zi;
                  r = mq_dot(Dl + e * ld, zv, n) - lam * zi + s - ddv[e];
                  w = lam / (s + rz * lam);
                  bs = w * (r + rz * lam);
                }
                rinv[e] = r; wv_[e] = w; bsv[e] = bs;
                RIN[(size_t)j * nd + e] = r;
                a_rp = cl_absmax(a_rp, r / fmax(1.0, fabs(ddv[e]))); a_lam = cl_absmax(a_lam, lam);
              } else if (e < m + nx) {
                const int r = e - m;
                double v = mq_dot(El + r * ld, zv, n) - xn[r];
                if (AFF) if (cof) v = (mq_dot(El + r * ld, zv, n) + cof[k * nx + r]) - xn[r];
                rdynv[r] = v; RDYN[(size_t)j * nx + r] = v;
                a_dyn = cl_absmax(a_dyn, v); a_x = cl_absmax(a_x, zv[r]);
              } else {
                const int i = e - m - nx;
                gq[i] = mq_dot(Hl + i * ld, zv, n) + qv[i];
              }
            }
            if (EQ) for (int e = tid; e < me; e += LQR_NT) {                 // J z - r, and nu + (1 / rho)(J z - r) in the place of r
              const double r = mq_dot(Jl + e * ld, zv, n) - rrv[e];
              a_rp = cl_absmax(a_rp, r / fmax(1.0, fabs(rrv[e])));
              reqv[e] = r; REQ[(size_t)j * ne + e] = r;
              rrv[e] = nuev[e] + MQ_RINV * r;
            }
            if (tx < n) for (int r = ty; r < nx; r += rs) {
              double acc = 0.0;
              for (int c = 0; c < nx; ++c) acc = fma(Pl[r * ldp + c], El[c * ld + tx], acc);
              Wl[r * ld + tx] = acc;
            }
            __syncthreads();
            // ---- B: g = H z + q + D' lam, [pi_j; r_u] = g + E' pi_{j+1}, v = Pi r_dyn + p, Hb = H + E' Pi E + D' w D
            for (int e = tid; e < n + nx; e += LQR_NT) {
              if (e < n) {
                double dl = 0.0, db = 0.0, ep = 0.0;
                for (int r = 0; r < m; ++r) { const double x = Dl[r * ld + e]; dl = fma(x, lamv[r], dl); db = fma(x, bsv[r], db); }
                if (EQ) for (int r = 0; r < me; ++r) { const double x = Jl[r * ld + e]; dl = fma(x, nuev[r], dl); db = fma(x, rrv[r], db); }
                for (int r = 0; r < nx; ++r) ep = fma(El[r * ld + e], pin[r], ep);
                const double g = gq[e] + dl;
                a_g = cl_absmax(a_g, g);
                fullv[e] = g + ep;
                if (e >= nx) a_rd = cl_absmax(a_rd, g + ep);
                hp[e] = gq[e] + db;
              } else {
                const int r = e - n;
                vv[r] = mq_dot(Pl + r * ldp, rdynv, nx) + pv[r];
              }
            }
            if (!facfail && tx < n) for (int i = ty; i < n; i += rs) {
              double acc = Hl[i * ld + tx];
              for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + i], Wl[r * ld + tx], acc);
              for (int r = 0; r < m; ++r) acc = fma(Dl[r * ld + i] * wv_[r], Dl[r * ld + tx], acc);
              if (EQ) for (int r = 0; r < me; ++r) acc = fma(Jl[r * ld + i] * MQ_RINV, Jl[r * ld + tx], acc);
              Hl[i * ld + tx] = acc;
            }
            __syncthreads();
            // ---- C: h = H z + q + D' (w (r_in + rho lam)) + E' v; its u part becomes column n of Hb; pi_j
            if (tid < n) {
              double acc = hp[tid];
              for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + tid], vv[r], acc);
              hp[tid] = acc;
              if (tid >= nx) Hl[tid * ld + n] = acc;
              else pin[tid] = fullv[tid];
            }
            __syncthreads();
            if (!facfail) {
              // ---- S = R' R in the rows nx .. n-1 of Hb, the right-hand sides [Hb_ux | h_u] along: one pivot per barrier, rows scaled at the end
              for (int c = 0; c < mb; ++c) {
                const double piv = Hl[(nx + c) * ld + nx + c];
                if (!(piv > 0.0 && piv < INFINITY)) { facfail = 1; break; }
                pivmin = fmin(pivmin, piv);
                const double inv = 1.0 / piv;
                const double* prow = Hl + (nx + c) * ld;
                for (int i = c + 1 + ty; i < mb; i += rs) {
                  const double f = prow[nx + i] * inv;
                  double* row = Hl + (nx + i) * ld;
                  for (int col = tx; col <= n; col += cw) if (col < nx || col > nx + c) row[col] = fma(-f, prow[col], row[col]);
                }
                __syncthreads();
              }
            }
            if (!facfail) {
              if (tid < mb) dgv[tid] = 1.0 / sqrt(Hl[(nx + tid) * ld + nx + tid]);
              __syncthreads();
              for (int i = ty; i < mb; i += rs) {
                const double sc = dgv[i];
                for (int col = tx; col <= n; col += cw) {
                  const double v = Hl[(nx + i) * ld + col] * sc;
                  Hl[(nx + i) * ld + col] = v;
                  FAC[(size_t)j * fs + i * (n + 1) + col] = v;
                }
              }
              __syncthreads();
              // ---- Pi_j = sym(Hb_xx) - Y' Y,  p_j = h_x - Y' y
              if (tx < nx) for (int i = ty; i < nx; i += rs) {
                double acc = 0.5 * (Hl[i * ld + tx] + Hl[tx * ld + i]);
                for (int c = 0; c < mb; ++c) acc = fma(-Hl[(nx + c) * ld + i], Hl[(nx + c) * ld + tx], acc);
                Pl[i * ldp + tx] = acc;
              }
              if (tid >= 64 && tid < 64 + nx) {
                const int r = tid - 64;
                double acc = hp[r];
                for (int c = 0; c < mb; ++c) acc = fma(-Hl[(nx + c) * ld + r], Hl[(nx + c) * ld + n], acc);
                pv[r] = acc;
              }
            }
            __syncthreads();
          }
          // ---- the figures of the iterate and the stop test
          double part = 0.0;
          for (int e = tid; e < N * nd; e += LQR_NT) part = fma(Lg[e], Sg[e], part);
          if (SOFT) for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) part = fma(Eg[e], NUg[e], part);
          const double sumc = mq_block<0>(part, red, tid);
          const double xmax = mq_block<1>(a_x, red, tid), lmax = mq_block<1>(a_lam, red, tid), gmax = mq_block<1>(a_g, red, tid);
          rp = fmax(mq_block<1>(a_rp, red, tid), mq_block<1>(a_dyn, red, tid) / fmax(1.0, xmax));
          if (EQ) rp = fmax(rp, mq_block<1>(tid < nt ? cl_absmax(0.0, tv[tid]) : 0.0, red, tid) / fmax(1.0, xmax));      // (tv: still Tx x_N of this pass)
          rd = mq_block<1>(a_rd, red, tid) / fmax(1.0, gmax);
          mu = mt > 0 ? sumc / mp : 0.0;
          if (!(rp < INFINITY && rd < INFINITY && fabs(mu) < INFINITY && lmax < INFINITY && xmax < INFINITY)) { status = MQ_NONFINITE; break; }
          if (rp <= tol && rd <= tol && mu <= MQ_MU_FACTOR * tol * fmax(1.0, lmax)) break;
          if (facfail) { status = MQ_NOT_CONVEX; break; }
          if (it == max_iter) { status = MQ_MAXITER; break; }

          double alpha = 1.0;
          for (int sweep = 0; sweep < 2; ++sweep) {
            if (sweep == 1) {
              if (mt == 0) break;
              // ============================================================== the corrector: sigma, c, and the change of y swept backward
              const double aa = fmin(1.0, alpha);
              part = 0.0;
              for (int e = tid; e < N * nd; e += LQR_NT) part = fma(Lg[e] + aa * dLg[e], Sg[e] + aa * dSg[e], part);
              if (SOFT) for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) {
                if (QUAD && zq_at(e) > 0.0) { MQ_QUAD_BLOCK; part = fma(Eg[e] + aa * dEg[e], NUg[e] + aa * (zq_at(e) * dEg[e] - dLg[e]), part); }      // dnu = Z de - dlam
                else part = fma(Eg[e] + aa * dEg[e], NUg[e] - aa * dLg[e], part);
              }
              const double r3 = mq_block<0>(part, red, tid) / mp / mu;
              const double sigmu = r3 * r3 * r3 * mu;
              for (int e = tid; e < N * nd; e += LQR_NT) {
                const int j = e / nd, i = e - j * nd;
                COR[e] = i < rows_of((k0s + j % p) % p) ? (sigmu - dSg[e] * dLg[e]) / (Sg[e] + MQ_RHO * Lg[e]) : 0.0;
                if (SOFT) if (soft_at(e)) {                                  // w (c1 / lam - c2 / nu), and c2 / nu for the forward sweep
                  double c2 = (sigmu + dEg[e] * dLg[e]) / NUg[e];
                  COR[e] = ((sigmu - dSg[e] * dLg[e]) / Lg[e] - c2) / (Sg[e] / Lg[e] + Eg[e] / NUg[e] + MQ_RHO);
                  if (QUAD) if (zq_at(e) > 0.0) {                            // c2 = sigma mu - de_aff dnu_aff, over nut
                    MQ_QUAD_BLOCK;
                    const double z = zq_at(e), nut = NUg[e] + z * Eg[e];
                    c2 = (sigmu - dEg[e] * (z * dEg[e] - dLg[e])) / nut;
                    COR[e] = ((sigmu - dSg[e] * dLg[e]) / Lg[e] - c2) / (Sg[e] / Lg[e] + Eg[e] / nut + MQ_RHO);
                  }
                  C2g[e] = c2;
                }
                if (QUAD) if (pure_at(e)) { MQ_QUAD_BLOCK; COR[e] = (sigmu - dSg[e] * dLg[e]) / (Sg[e] + (MQ_RHO + 1.0 / zq_at(e)) * Lg[e]); }
              }
              if (tid < nx) dxa[tid] = 0.0;                                  // dp_N
              __syncthreads();
              double* dp = dxa; double* dpn = dxb;
              for (int j = N - 1; j >= 0; --j) {
                const int k = (k0s + j % p) % p, m = rows_of(k);
                mq_fetch(El, nullptr, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, nullptr, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
                for (int i = ty; i < mb; i += rs) for (int col = tx; col <= n; col += cw) Hl[(nx + i) * ld + col] = FAC[(size_t)j * fs + i * (n + 1) + col];
                for (int i = tid; i < m; i += LQR_NT) corv[i] = COR[(size_t)j * nd + i];
                __syncthreads();
                if (tid < n) {
                  double acc = 0.0;
                  for (int r = 0; r < m; ++r) acc = fma(Dl[r * ld + tid], corv[r], acc);
                  for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + tid], dp[r], acc);
                  hp[tid] = acc;
                }
                __syncthreads();
                if (wave == 0) {                                             // R' dy = dh_u, column by column inside one wave
                  double tt = lane < mb ? hp[nx + lane] : 0.0;
                  for (int c = 0; c < mb; ++c) {
                    const double yc = __shfl(tt, c, 64) / Hl[(nx + c) * ld + nx + c];
                    if (lane > c && lane < mb) tt = fma(-Hl[(nx + c) * ld + nx + lane], yc, tt);
                    if (lane == c) tt = yc;
                  }
                  if (lane < mb) { dyv[lane] = tt; FAC[(size_t)j * fs + lane * (n + 1) + n] = Hl[(nx + lane) * ld + n] + tt; }
                }
                __syncthreads();
                if (tid < nx) {
                  double acc = hp[tid];
                  for (int c = 0; c < mb; ++c) acc = fma(-Hl[(nx + c) * ld + tid], dyv[c], acc);
                  dpn[tid] = acc;
                }
                __syncthreads();
                { double* t_ = dp; dp = dpn; dpn = t_; }
              }
            }
            // ================================================================ the forward sweep: the direction and its largest step
            if (tid < nx) dxa[tid] = 0.0;
            __syncthreads();
            double* dx = dxa; double* dxn = dxb;
            double amin = 1e300;
            const bool last = EQ && (sweep == 1 || mt == 0);                 // (EQ) the sweep whose direction is taken: it computes dnu
            for (int j = 0; j < N; ++j) {
              const int k = (k0s + j % p) % p, m = rows_of(k);
              const int me = last ? erows_of(k) : 0;
              if (EQ) if (last) {
                if (tx < n) for (int i = ty; i < me; i += rs) Jl[i * ld + tx] = J[((size_t)k * ne + i) * n + tx];
                for (int i = tid; i < me; i += LQR_NT) reqv[i] = REQ[(size_t)j * ne + i];
              }
              mq_fetch(El, nullptr, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, nullptr, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
              for (int i = ty; i < mb; i += rs) for (int col = tx; col <= n; col += cw) Hl[(nx + i) * ld + col] = FAC[(size_t)j * fs + i * (n + 1) + col];
              for (int i = tid; i < m; i += LQR_NT) {
                lamv[i] = Lg[(size_t)j * nd + i]; sv[i] = Sg[(size_t)j * nd + i]; rinv[i] = RIN[(size_t)j * nd + i]; corv[i] = sweep ? COR[(size_t)j * nd + i] : 0.0;
              }
              if (SOFT) for (int i = tid; i < m; i += LQR_NT) { ev[i] = Eg[(size_t)j * nd + i]; nuv[i] = NUg[(size_t)j * nd + i]; cv[i] = pen[k * nd + i]; }
              if (QUAD) for (int i = tid; i < m; i += LQR_NT) zqv[i] = pen2[k * nd + i];
              if (tid >= 64 && tid < 64 + nx) rdynv[tid - 64] = RDYN[(size_t)j * nx + tid - 64];
              __syncthreads();
              if (wave == 0) {                                               // du = -R^-1 (Y dx + y), column by column inside one wave
                double tt = lane < mb ? mq_dot(Hl + (nx + lane) * ld, dx, nx) + Hl[(nx + lane) * ld + n] : 0.0;
                for (int c = mb - 1; c >= 0; --c) {
                  const double uc = __shfl(tt, c, 64) / Hl[(nx + c) * ld + nx + c];
                  if (lane < c) tt = fma(-Hl[(nx + lane) * ld + nx + c], uc, tt);
                  if (lane == c) tt = uc;
                }
                if (lane < mb) { dzv[nx + lane] = -tt; dZ[(size_t)j * n + nx + lane] = -tt; }
              } else if (tid - 64 < nx) {
                const double v = dx[tid - 64];
                dzv[tid - 64] = v; dZ[(size_t)j * n + tid - 64] = v;
              }
              __syncthreads();
              for (int e = tid; e < m + nx; e += LQR_NT) {
                if (e < m) {
                  const double lam = lamv[e], s = sv[e], Dz = mq_dot(Dl + e * ld, dzv, n);
                  const double w = lam / (s + MQ_RHO * lam);
                  double dl = corv[e] - w * s + w * (rinv[e] + Dz);
                  double ds = -rinv[e] - Dz + MQ_RHO * dl;
                  if (SOFT) if (cv[e] < INFINITY) if (!QUAD || (cv[e] > 0.0 && !(zqv[e] > 0.0))) {
                    const double ee = ev[e], nu = nuv[e];
                    const double ws_ = 1.0 / (s / lam + ee / nu + MQ_RHO);
                    dl = corv[e] + ws_ * (rinv[e] - s + ee + Dz);
                    const double de = -ee + (sweep ? C2g[(size_t)j * nd + e] : 0.0) + (ee / nu) * dl;
                    ds = -rinv[e] - Dz + de + MQ_RHO * dl;
                    dEg[(size_t)j * nd + e] = de;
                    if (de < 0.0) amin = fmin(amin, -ee / de);
                    if (dl > 0.0) amin = fmin(amin, nu / dl);                // dnu = -dlam
                  }
                  if (QUAD) if (cv[e] < INFINITY && cv[e] > 0.0 && zqv[e] > 0.0) {      // L1 + L2: de = (c2 - e nu + e dlam) / nut, dnu = Z de - dlam
                    MQ_QUAD_BLOCK;
                    const double ee = ev[e], nu = nuv[e], nut = nu + zqv[e] * ee, enu = ee * nu / nut;
                    const double ws_ = 1.0 / (s / lam + ee / nut + MQ_RHO);
                    dl = corv[e] + ws_ * (rinv[e] - s + enu + Dz);
                    const double de = -enu + (sweep ? C2g[(size_t)j * nd + e] : 0.0) + (ee / nut) * dl;
                    ds = -rinv[e] - Dz + de + MQ_RHO * dl;
                    dEg[(size_t)j * nd + e] = de;
                    const double dnu = zqv[e] * de - dl;
                    if (de < 0.0) amin = fmin(amin, -ee / de);
                    if (dnu < 0.0) amin = fmin(amin, -nu / dnu);
                  }
                  if (QUAD) if (cv[e] == 0.0) {                              // pure quadratic: the hard row with rho + 1 / Z
                    MQ_QUAD_BLOCK;
                    const double rz = MQ_RHO + 1.0 / zqv[e], wz = lam / (s + rz * lam);
                    dl = corv[e] - wz * s + wz * (rinv[e] + Dz);
                    ds = -rinv[e] - Dz + rz * dl;
                  }
                  dLg[(size_t)j * nd + e] = dl; dSg[(size_t)j * nd + e] = ds;
                  if (ds < 0.0) amin = fmin(amin, -s / ds);
                  if (dl < 0.0) amin = fmin(amin, -lam / dl);
                } else {
                  const int r = e - m;
                  dxn[r] = mq_dot(El + r * ld, dzv, n) + rdynv[r];
                }
              }
              if (EQ) for (int e = tid; e < me; e += LQR_NT) REQ[(size_t)j * ne + e] = MQ_RINV * (mq_dot(Jl + e * ld, dzv, n) + reqv[e]);     // dnu
              __syncthreads();
              { double* t_ = dx; dx = dxn; dxn = t_; }
            }
            if (tid < nx) dZ[(size_t)N * n + tid] = dx[tid];
            if (EQ) if (last && tid < nt) {                                  // dnu_T
              double acc = 0.0;
              for (int c = 0; c < nx; ++c) acc = fma(tx_at(tid, c), dx[c], acc);
              tv[tid] = MQ_RINV * (acc + tv[tid]);
            }
            alpha = mq_block<2>(amin, red, tid);
          }
          // ================================================================ the step
          const double al = fmin(1.0, MQ_STEP_BACK * alpha);
          for (int e = tid; e < (N + 1) * n; e += LQR_NT) Z[e] = fma(al, dZ[e], Z[e]);
          if (SOFT) for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) {
            if (QUAD && zq_at(e) > 0.0) { MQ_QUAD_BLOCK; NUg[e] = fma(al, zq_at(e) * dEg[e] - dLg[e], NUg[e]); Eg[e] = fma(al, dEg[e], Eg[e]); }
            else { Eg[e] = fma(al, dEg[e], Eg[e]); NUg[e] = fma(-al, dLg[e], NUg[e]); }
          }
          for (int e = tid; e < N * nd; e += LQR_NT) { Sg[e] = fma(al, dSg[e], Sg[e]); Lg[e] = fma(al, dLg[e], Lg[e]); }
          if (EQ) {
            for (int e = tid; e < N * ne; e += LQR_NT) NUe[e] = fma(al, REQ[e], NUe[e]);
            if (tid < nt) NUT[tid] = fma(al, tv[tid], NUT[tid]);
          }
          __syncthreads();
        }
        if (WARM) {
          // a warm attempt that ran out of iterations or met a stage matrix that is not positive definite: the same step again from the cold start, its
          // iterations added (an infeasible instance costs two runs of max_iter); status 3 is not retried
          if (warm_now && (status == MQ_MAXITER || status == MQ_NOT_CONVEX)) {
            status = MQ_OK; its_warm = its; warm_now = false; retried = true;
            __syncthreads();
            goto mq_start;
          }
          its += its_warm;
          wcode = status == MQ_OK ? (retried ? 2 : (warm_now ? 1 : 0)) : -1;
        }
        it_total += its; it_max = max(it_max, its);
      }
      // ---- the step's results: u_0, the open-loop solution of step 0, nact, hres, x <- E [x; u_0]
      const bool ok = status == MQ_OK && done == t;
      if (ok) {
        const int m = rows_of(k0s);
        mq_fetch(El, nullptr, Dl, ld, (AFF ? Ap : A) + (size_t)k0s * nx * nx, (AFF ? Bp : B) + (size_t)k0s * nx * mb, nullptr, D ? D + (size_t)k0s * nd * n : nullptr, nx, mb,
                 m, tx, ty, rs);
        if (tid < n) zv[tid] = Z[tid];
        const int me0 = EQ ? erows_of(k0s) : 0;
        if (EQ) if (tx < n) for (int i = ty; i < me0; i += rs) Jl[i * ld + tx] = J[((size_t)k0s * ne + i) * n + tx];
        __syncthreads();
        double hmax = -INFINITY, cnt = 0.0;
        for (int i = tid; i < m; i += LQR_NT) {
          hmax = fmax(hmax, mq_dot(Dl + i * ld, zv, n) - dd[k0s * nd + i]);
          if (Lg[i] > Sg[i]) cnt += 1.0;
        }
        hres = mq_block<1>(hmax, red, tid);
        nact = (int)mq_block<0>(cnt, red, tid);
        if (SOFT) {
          double cv_ = 0.0;
          for (int i = tid; i < m; i += LQR_NT) if (Eg[i] > NUg[i]) cv_ += 1.0;
          if (QUAD) for (int i = tid; i < m; i += LQR_NT) if (pen[k0s * nd + i] == 0.0 && Lg[i] > Sg[i]) cv_ += 1.0;      // a pure row: active is violated
          nviol = (int)mq_block<0>(cv_, red, tid);
          if (!QUAD) if (t == 0 && Eolg) for (int e = tid; e < N * nd; e += LQR_NT) Eolg[((b * ns + si) * N) * nd + e] = Eg[e];
          if (QUAD) if (t == 0 && Eolg) for (int e = tid; e < N * nd; e += LQR_NT) {      // e = lam / Z on a pure row
            const int j = e / nd, i = e - j * nd, k = (k0s + j % p) % p;
            Eolg[((b * ns + si) * N) * nd + e] = i < rows_of(k) && pen[k * nd + i] == 0.0 ? Lg[e] / pen2[k * nd + i] : Eg[e];
          }
        }
        if (EQ) {
          double em = 0.0;
          for (int i = tid; i < me0; i += LQR_NT) em = cl_absmax(em, mq_dot(Jl + i * ld, zv, n) - (rq ? rq[k0s * ne + i] : 0.0));
          eres = mq_block<1>(em, red, tid);
          if (t == 0) {
            if (Nug) for (int e = tid; e < N * ne; e += LQR_NT) Nug[((b * ns + si) * N) * ne + e] = NUe[e];
            if (NuTg && tid < nt) NuTg[(b * ns + si) * nt + tid] = NUT[tid];
          }
        }
        if (t == 0) {
          if (Xolg) for (int e = tid; e < (N + 1) * nx; e += LQR_NT) { const int j = e / nx; Xolg[((b * ns + si) * (N + 1)) * nx + e] = Z[(size_t)j * n + e - j * nx]; }
          if (Uolg) for (int e = tid; e < N * mb; e += LQR_NT) { const int j = e / mb; Uolg[((b * ns + si) * N) * mb + e] = Z[(size_t)j * n + nx + e - j * mb]; }
          if (Lamg) for (int e = tid; e < N * nd; e += LQR_NT) Lamg[((b * ns + si) * N) * nd + e] = Lg[e];
        }
        double xnew = 0.0;
        if (tid < nx) xnew = mq_dot(El + tid * ld, zv, n);
        if (AFF) if (tid < nx) {                                             // the plant's offset and the disturbance of this step
          if (cpl) xnew += cpl[k0s * nx + tid];
          if (Wd) xnew += Wd[(size_t)t * nx + tid];
        }
        if (tid >= 64 && tid < 64 + mb) {
          const double u = zv[nx + tid - 64];
          if (t == 0) U0g[(b * ns + si) * mb + tid - 64] = u;
          if (Ug) Ug[((b * T + t) * ns + si) * mb + tid - 64] = u;
        }
        __syncthreads();
        if (tid < nx) {
          xcur[tid] = xnew;
          if (Xg) Xg[((b * (T + 1) + t + 1) * ns + si) * nx + tid] = xnew;
        }
        __syncthreads();
        done = t + 1;
      } else {
        if (tid < mb) {
          if (t == 0) U0g[(b * ns + si) * mb + tid] = qnan;
          if (Ug) Ug[((b * T + t) * ns + si) * mb + tid] = qnan;
        }
        if (tid < nx && Xg) Xg[((b * (T + 1) + t + 1) * ns + si) * nx + tid] = qnan;
        if (t == 0) {
          if (Xolg) for (int e = tid; e < (N + 1) * nx; e += LQR_NT) Xolg[((b * ns + si) * (N + 1)) * nx + e] = qnan;
          if (Uolg) for (int e = tid; e < N * mb; e += LQR_NT) Uolg[((b * ns + si) * N) * mb + e] = qnan;
          if (Lamg) for (int e = tid; e < N * nd; e += LQR_NT) Lamg[((b * ns + si) * N) * nd + e] = qnan;
          if (SOFT) if (Eolg) for (int e = tid; e < N * nd; e += LQR_NT) Eolg[((b * ns + si) * N) * nd + e] = qnan;
          if (EQ) {
            if (Nug) for (int e = tid; e < N * ne; e += LQR_NT) Nug[((b * ns + si) * N) * ne + e] = qnan;
            if (NuTg && tid < nt) NuTg[(b * ns + si) * nt + tid] = qnan;
          }
        }
      }
      if (tid == 0) {
        const size_t o = (b * T + t) * ns + si;
        if (itersg) itersg[o] = done >= t ? its : -1;
        if (nactg) nactg[o] = nact;
        if (hresg) hresg[o] = hres;
        if (SOFT) if (nviolg) nviolg[o] = nviol;
        if (EQ) if (eresg) eresg[o] = eres;
        if (WARM) if (wm.log) wm.log[o] = done > t ? wcode : -1;
      }
    }
    if (tid < nx) XTg[(b * ns + si) * nx + tid] = status == MQ_OK ? xcur[tid] : qnan;
    if (tid == 0) {
      double* o = infog + (b * ns + si) * MQ_INFO;
      o[0] = status; o[1] = done; o[2] = it_total; o[3] = it_max; o[4] = mu; o[5] = rp; o[6] = rd; o[7] = pivmin;
    }
    __syncthreads();
  }
}

// The six instantiations without quadratic penalties by the three parameters they have always had (the launch table of tmpc_api.hip names them so).
template <bool SOFT, bool EQ, bool AFF>
constexpr auto mpc_qp_kernel() { return &k_mpc_qp<SOFT, EQ, AFF, false>; }

}  // namespace tmpc
