// The periodic optimal-control QP (the LQ case of the reference's pocp.py, the subproblem of its sqp_method.Sqp): the orbit that the MPC entries take as
// their reference.  Per problem, with N = periods p and k = k_j = j mod p,
//   min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j),   z_j = [x_j; u_j],
//   s.t. x_{j+1} = A_k x_j + B_k u_j + c_k,  j = 0 .. N-1,  x_N := x_0  (x_0 is a variable),
//        D_k z_j <= d_k (first ndcnt_k rows),   J_k z_j = r_k (first necnt_k rows).
// Not served: warm starts, a terminal cost (Pf has no meaning without an end), the phase-fixing cost of pocp.py.  Soft and quadratic-slack rows are served
// by the SOFT instantiation (below).
//
// Conventions: those stated at the top of tmpc_mpc_qp.h -- one 256-thread workgroup per problem, fp64 on the vector ALU, the whole interior-point loop in
// one launch, the operands of a stage in LDS, per-stage factors and the iterate in a slot of a global workspace, min(nb, MQ_SLOTS) workgroups that loop over
// the problems, every sum in a fixed order that depends on nothing but the problem, uniform control flow with no exit around a barrier.  mq_dot, mq_block
// and mq_fetch are that header's.
//
// Iteration: the hard / EQ / AFF one of tmpc_mpc_qp.h, rule by rule (tests/periodic_qp_reference.py states the same rules on the dense problem): start z = 0
// including x_0, s = max(d, 1), lam = 1, nu = 0; w = lam / (s + rho lam), equality rows at the weight 1 / rho; Mehrotra with sigma = (mu_aff / mu)^3; one
// step length min(1, 0.995 alpha_max); the stop rule and its scales.  What the periodic boundary changes:
//   pi_per     the multiplier of x_N = x_0 is a VARIABLE (start 0; it moves with the step length): I - (A_{N-1} .. A_0)' may be singular, so it cannot be
//              derived from the iterate.  The other multipliers of the dynamics stay the adjoint of the iterate, started from pi_N = pi_per;
//   residuals  the dual residual has one more block, the x_0 rows (H z_0 + q + D' lam + J' nu)_x + A_0' pi_1 - pi_per; the dynamics residual of the last
//              stage is E z_{N-1} + c - x_0 (x_N is not stored).
// Newton step (the block-cyclic system is the acyclic one plus a border of nx columns, as k_solve_border does it for the main solver):
//   pass 1     the Riccati pass of tmpc_mpc_qp.h from Pi_N = 0, p_N = pi_per.  In the same pass nx border columns are swept backward with its factors:
//              M_N = I,  T = E' M_{j+1},  Gy_j = R^-T T_u,  M_j = T_x - Y' Gy_j   (the corrector's sweep dh = E' dp, dy = R^-T dh_u, dp = dh_x - Y' dy
//              on the columns of I), so that p_j(p_N + dpi) = p_j + M_j dpi and y_j(..) = y_j + Gy_j dpi, and along the way
//              Gamma = sum_j Gy_j' Gy_j,   phi = sum_j (M_{j+1}' r_dyn,j - Gy_j' y_j):
//              forward, the closed loop gives dx_N = M_0' dx_0 + phi - Gamma dpi;
//   border     the two boundary conditions (stationarity in x_0: Pi_0 dx_0 + p_0 + M_0 dpi = pi_per + dpi; periodicity: dx_N = dx_0) are one symmetric
//              quasi-definite system of size 2 nx, with a = p_0 - pi_per:
//                  [ Pi_0       M_0 - I ] [dx_0]     [ a   ]
//                  [ M_0' - I   -Gamma  ] [dpi ] = - [ phi ]
//              solved by Pi_0 = R0' R0 (elimination along [Pi_0 | M_0 - I], W = R0^-T (M_0 - I)) and S = Gamma + W' W = R2' R2:
//              dpi = S^-1 (phi - W' R0^-T a),  dx_0 = -R0^-1 (R0^-T a + W dpi).  A pivot of either that is not positive and finite is status 2 (pivmin takes
//              these pivots too): Pi_0 not positive definite, or no unique periodic trajectory (A = I, B = 0: M_0 = I, Gamma = 0, S = 0 exactly);
//   sweep      the forward sweep of tmpc_mpc_qp.h from dx_0 with du = -R^-1 (Y dx + y + Gy_j dpi);
//   corrector  only right-hand sides: the backward sweep of the change of y ends in da = dp_0 and collects dphi = -sum_j Gy_j' dy_j; the border columns,
//              R0, W and R2 are those of the predictor.
// Statuses: 0 converged, 1 max_iter reached (contradictory rows end here), 2 a stage matrix S, Pi_0 or the border's S not positive definite (a problem with
// no periodic trajectory ends here or with 1, never with 0), 3 non-finite.  A problem that fails returns NaN in X, U, Lam, Nu, Pi and res.
//
// LDS (periodic_qp_lds): the hard / EQ layout of tmpc_mpc_qp.h, then M [nx x ldp] (M_{j+1}, then W), T [n x ldp], Gamma [nx x ldp] (then R2),
// Gy [mb x ldp] and PQ_NVEC vectors of ldp doubles, ldp = nx | 1; R0 lies where Pi_0 lay.  Two shapes, in bytes: nx 24 / nu 8 / nd 16 / ne 0: 56144;
// nx 3 / nu 2 / nd 4 / ne 1: 2760.  Workspace per slot (periodic_qp_ws_doubles): the hard / EQ workspace with nt = 0, then GY [N][mb][nx] and PI [N][nx]
// (PI[0] is pi_per, PI[j] the adjoint pi_j of the last pass 1).
//
// Soft and quadratic-slack rows (k_periodic_qp<true>; the reference's pocp.py carries slacked constraints, sys['g'] and the us variables).  The row kind is
// read per row from c = penalty and Z = penalty2, as the QUAD instantiations of tmpc_mpc_qp.h read it (tests/periodic_qp_soft_reference.py states the same
// rules on the dense problem):
//   c = inf (Z = 0)  the hard row;      c > 0, Z = 0  exact L1 (D_i z - e <= d, e >= 0, cost c e);      c > 0, Z > 0  L1 + L2 (cost c e + 1/2 Z e^2, stationarity
//   c + Z e - lam - nu = 0);      c = 0, Z > 0  pure quadratic, one pair, a hard row with the dual regularisation rho + 1 / Z, slack lam / Z.
// Taken from the "Soft rows" and "Quadratic slack penalties" sections of tmpc_mpc_qp.h unchanged: the start values, r_in, the weights w and beta, the corrector
// terms c1 / c2, dnu = Z de - dlam, mu and sigma over every pair once, the step length over s, lam, e, nu, the stop rule with max lam over lam alone.
// Where they stand here: pass 1 block A (row residual, w, bsv), so block B (hp and the D' w D term of Hb) reads them as it read the hard ones; the corrector
// (the COR column, C2 = c2 / nu or c2 / nut for the forward sweep); the forward sweep (dlam, ds, de, amin); the step and the start block.
// The border is untouched: M, T, Gamma, Gy, phi, R0, W, R2 and border_solve see a soft row only through a row's weight and right-hand side.
// Invalid weights (c negative or NaN; Z negative or non-finite; Z != 0 on a hard row; c = 0 with Z = 0) give status 3 before the first iteration.
// Outputs: Eps [nb][N][nd] (e; lam / Z on a pure row; 0 on hard and absent rows), nviol [nb] (over all N stages the two-pair rows with e > nu plus the pure
// rows with lam > s), res [nb][6] = cost, hres, eres, per, pcost, emax: pcost = sum c e + 1/2 Z e^2 over the reported slacks, cost includes it, emax is their
// maximum, hres stays max(D z - d).  A failed problem returns NaN in the floating-point outputs and -1 in nviol.
// LDS (periodic_qp_soft_lds): the order of mpc_qp_quad_eq_layout -- the hard layout, the vectors e, nu, c, Z of the stage [nd] each, the EQ part -- then the
// border as above: 32 nd bytes more than periodic_qp_lds.  The soft layout of the two shapes above, in bytes: 56656 and 2888.  Workspace
// (periodic_qp_soft_ws_doubles): E, NU, dE, C2 [N][nd] each after FAC, then NUe, REQ, GY, PI: 4 N nd doubles more; nx 24 / nu 8 / nd 16 / ne 0 / N 6: 4432
// doubles, nx 3 / nu 2 / nd 4 / ne 1 / N 3: 238.
// With SOFT = false the kernel is the one it was, statement by statement: every statement of SOFT stands behind `if (SOFT)` or is a value selected by it at
// compile time; MQ_QUAD_BLOCK keeps the blocks of the rows with Z > 0 apart from the statements beside them.
#pragma once
#include "tmpc_mpc_qp.h"

namespace tmpc {

constexpr int PQ_INFO = 8;                   // doubles of info per problem: the fields of MQ_INFO (TMPC_PERIODIC_QP_INFO)
constexpr int PQ_RES = 4;                    // doubles of res per problem: cost, hres, eres, per (TMPC_PERIODIC_QP_RES)
constexpr int PQ_RES_SOFT = 6;               // the soft entries: cost (pcost included), hres, eres, per, pcost, emax (TMPC_PERIODIC_QP_SOFT_RES)
constexpr int PQ_NVEC = 10;                  // vector slots of the border (seven in use: pi_per, dpi, dx_0, a and phi of the predictor and of the corrector)

struct PeriodicQpLds { MpcQpEqLds e; int ldp, oM, oT, oG, oGy, oBv, total; };      // offsets in doubles
__host__ __device__ inline PeriodicQpLds periodic_qp_lds(int nx, int mb, int nd, int ne) {
  PeriodicQpLds l;
  l.e = mpc_qp_eq_lds(nx, mb, nd, ne, false);
  l.ldp = nx | 1;
  const long long ldp = l.ldp, oM = l.e.total, oT = oM + nx * ldp, oG = oT + (long long)(nx + mb) * ldp, oGy = oG + nx * ldp, oBv = oGy + mb * ldp;
  const long long total = oBv + PQ_NVEC * ldp;
  const bool big = total > 0x7fffffffLL / 8;
  l.oM = big ? 0 : (int)oM; l.oT = big ? 0 : (int)oT; l.oG = big ? 0 : (int)oG; l.oGy = big ? 0 : (int)oGy; l.oBv = big ? 0 : (int)oBv;
  l.total = big ? 0x7fffffff / 8 : (int)total;
  return l;
}
__host__ __device__ inline long long periodic_qp_ws_doubles(int nx, int mb, int nd, int ne, int N) {
  return mpc_qp_eq_ws_doubles(nx, mb, nd, N, ne, 0, false) + (long long)N * mb * nx + (long long)N * nx;
}

// The SOFT instantiation: the layout of mpc_qp_quad_eq_layout (the hard layout, the vectors e, nu, c, Z of the stage [nd] each, then the EQ part), then the
// border as above; the workspace of the soft EQ kernel (E, NU, dE, C2 [N][nd] each after FAC, then NUe, REQ), then GY and PI.
__host__ __device__ inline PeriodicQpLds periodic_qp_soft_lds(int nx, int mb, int nd, int ne) {
  PeriodicQpLds l;
  l.e = mpc_qp_quad_eq_layout(nx, mb, nd, ne);
  l.ldp = nx | 1;
  const long long ldp = l.ldp, oM = l.e.total, oT = oM + nx * ldp, oG = oT + (long long)(nx + mb) * ldp, oGy = oG + nx * ldp, oBv = oGy + mb * ldp;
  const long long total = oBv + PQ_NVEC * ldp;
  const bool big = total > 0x7fffffffLL / 8;
  l.oM = big ? 0 : (int)oM; l.oT = big ? 0 : (int)oT; l.oG = big ? 0 : (int)oG; l.oGy = big ? 0 : (int)oGy; l.oBv = big ? 0 : (int)oBv;
  l.total = big ? 0x7fffffff / 8 : (int)total;
  return l;
}
__host__ __device__ inline long long periodic_qp_soft_ws_doubles(int nx, int mb, int nd, int ne, int N) {
  return mpc_qp_eq_ws_doubles(nx, mb, nd, N, ne, 0, true) + (long long)N * mb * nx + (long long)N * nx;
}

// A [nb][p][nx][nx], B [nb][p][nx][mb], H [nb][p][n][n]; each or null: q [nb][p][n], c [nb][p][nx], D [nb][p][nd][n] and d [nb][p][nd] (null when nd = 0),
// ndcnt [nb][p] (null: all nd rows; clamped to 0 .. nd), J [nb][p][ne][n] (null when ne = 0), r [nb][p][ne] (null: zero), necnt [nb][p] (null: all ne rows;
// clamped).  ws: gridDim.x slots of periodic_qp_ws_doubles.  Outputs: info [nb][8]; each or null: X [nb][N][nx], U [nb][N][mb], Lam [nb][N][nd],
// Nu [nb][N][ne], Pi [nb][N][nx], res [nb][4].  cw = 1 << lcw: power of two >= n (<= 64).
struct PeriodicQpArgs {
  int p, nx, mb, nd, ne, N, lcw, max_iter;
  long long nb;
  double tol;
  const double* A; const double* B; const double* H; const double* q; const double* c; const double* D; const int* ndcnt; const double* d;
  const double* J; const double* r; const int* necnt;
  double* ws; double* X; double* U; double* Lam; double* Nu; double* Pi; double* info; double* res;
  const double* pen; const double* pen2; double* Eps; int* nviol;            // (SOFT) penalty, penalty2 [nb][p][nd] (one may be null), Eps [nb][N][nd], nviol [nb]; res [nb][6]
};

// grid: min(nb, MQ_SLOTS) workgroups.  SOFT: the instantiation with soft and quadratic-slack rows (the header comment); it reads pen, pen2 (one of them may
// be null) and writes Eps, nviol and six fields of res.  Without SOFT the four are not read or written and res has four fields.
template <bool SOFT>
__global__ void __launch_bounds__(LQR_NT) k_periodic_qp(PeriodicQpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int p = a.p, nx = a.nx, mb = a.mb, nd = a.nd, ne = a.ne, N = a.N, lcw = a.lcw, max_iter = a.max_iter;
  const double tol = a.tol;
  const int n = nx + mb;
  const MpcQpLds Ly = mpc_qp_lds(nx, mb, nd);
  const PeriodicQpLds Lp = SOFT ? periodic_qp_soft_lds(nx, mb, nd, ne) : periodic_qp_lds(nx, mb, nd, ne);
  const int ld = Ly.ld, ldp = Ly.ldp, lv = Ly.lv;
  double* El = lds + Ly.oE; double* Pl = lds + Ly.oP; double* Wl = lds + Ly.oW; double* Hl = lds + Ly.oH; double* Dl = lds + Ly.oD; double* red = lds + Ly.oR;
  double* V = lds + Ly.oV;
  double* zv = V; double* xn = V + lv; double* lamv = V + 2 * lv; double* sv = V + 3 * lv; double* ddv = V + 4 * lv; double* wv_ = V + 5 * lv;
  double* rinv = V + 6 * lv; double* bsv = V + 7 * lv; double* gq = V + 8 * lv; double* fullv = V + 9 * lv; double* hp = V + 10 * lv; double* rdynv = V + 11 * lv;
  double* vv = V + 12 * lv; double* pin = V + 13 * lv; double* pv = V + 14 * lv; double* dxa = V + 15 * lv; double* dxb = V + 16 * lv; double* dzv = V + 17 * lv;
  double* corv = V + 18 * lv; double* dgv = V + 20 * lv; double* dyv = V + 21 * lv; double* qv = V + 22 * lv;
  double* Jl = lds + Lp.e.oJ; double* nuev = lds + Lp.e.oNu; double* reqv = lds + Lp.e.oReq; double* rrv = lds + Lp.e.oR;
  // the border: M_{j+1} (then W), T, Gamma (then R2), Gy_j; pi_per, dpi, dx_0, a and phi of the predictor, a and phi of the corrector
  double* Ml = lds + Lp.oM; double* Tl = lds + Lp.oT; double* Gl = lds + Lp.oG; double* Gyl = lds + Lp.oGy; double* bv = lds + Lp.oBv;
  double* pip = bv; double* dpi = bv + ldp; double* dx0 = bv + 2 * ldp; double* av0 = bv + 3 * ldp; double* phiv = bv + 4 * ldp; double* av1 = bv + 5 * ldp;
  double* phic = bv + 6 * ldp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const long long wsn = SOFT ? periodic_qp_soft_ws_doubles(nx, mb, nd, ne, N) : periodic_qp_ws_doubles(nx, mb, nd, ne, N);
  double* ws = a.ws + (size_t)blockIdx.x * wsn;
  double* Z = ws; double* dZ = Z + (size_t)(N + 1) * n; double* Sg = dZ + (size_t)(N + 1) * n; double* Lg = Sg + (size_t)N * nd; double* dSg = Lg + (size_t)N * nd;
  double* dLg = dSg + (size_t)N * nd; double* RIN = dLg + (size_t)N * nd; double* COR = RIN + (size_t)N * nd; double* RDYN = COR + (size_t)N * nd;
  double* FAC = RDYN + (size_t)N * nx;
  const int fs = mb * (n + 1);                                               // doubles of [Y | R | y] per stage
  double* NUe = ws + (SOFT ? mpc_qp_soft_ws_doubles(nx, mb, nd, N) : mpc_qp_ws_doubles(nx, mb, nd, N)); double* REQ = NUe + (size_t)N * ne;
  double* GY = ws + mpc_qp_eq_ws_doubles(nx, mb, nd, N, ne, 0, SOFT); double* PI = GY + (size_t)N * mb * nx;
  double* Eg = FAC + (size_t)N * fs; double* NUg = Eg + (size_t)N * nd; double* dEg = NUg + (size_t)N * nd; double* C2g = dEg + (size_t)N * nd;   // (SOFT only)
  double* ev = lds + Ly.total; double* nuv = ev + nd; double* cv = nuv + nd; double* zqv = cv + nd;                                            // (SOFT only)

  // dx_0 and dpi of the right-hand sides aa (a) and ph (phi) with R0 (in Pl), W (in Ml) and R2 (in Gl): triangular solves column by column inside one wave
  auto border_solve = [&](const double* aa, const double* ph) {
    if (wave == 0) {
      const bool in = lane < nx;
      double w = in ? aa[lane] : 0.0;                                        // R0' w = a
      for (int c = 0; c < nx; ++c) {
        const double yc = __shfl(w, c, 64) / Pl[c * ldp + c];
        if (lane > c && in) w = fma(-Pl[c * ldp + lane], yc, w);
        if (lane == c) w = yc;
      }
      double t2 = in ? ph[lane] : 0.0;                                       // phi - W' w
      for (int i = 0; i < nx; ++i) {
        const double wi = __shfl(w, i, 64);
        if (in) t2 = fma(-Ml[i * ldp + lane], wi, t2);
      }
      for (int c = 0; c < nx; ++c) {                                         // R2' y = ..
        const double yc = __shfl(t2, c, 64) / Gl[c * ldp + c];
        if (lane > c && in) t2 = fma(-Gl[c * ldp + lane], yc, t2);
        if (lane == c) t2 = yc;
      }
      for (int c = nx - 1; c >= 0; --c) {                                    // R2 dpi = y
        const double xc = __shfl(t2, c, 64) / Gl[c * ldp + c];
        if (lane < c) t2 = fma(-Gl[lane * ldp + c], xc, t2);
        if (lane == c) t2 = xc;
      }
      double t3 = w;                                                         // R0 dx_0 = -(w + W dpi)
      for (int c = 0; c < nx; ++c) {
        const double dc = __shfl(t2, c, 64);
        if (in) t3 = fma(Ml[lane * ldp + c], dc, t3);
      }
      for (int c = nx - 1; c >= 0; --c) {
        const double xc = __shfl(t3, c, 64) / Pl[c * ldp + c];
        if (lane < c) t3 = fma(-Pl[lane * ldp + c], xc, t3);
        if (lane == c) t3 = xc;
      }
      if (in) { dpi[lane] = t2; dx0[lane] = -t3; }
    }
    __syncthreads();
  };

  for (long long b = blockIdx.x; b < a.nb; b += gridDim.x) {
    const double* A = a.A + (size_t)b * p * nx * nx; const double* B = a.B + (size_t)b * p * nx * mb; const double* H = a.H + (size_t)b * p * n * n;
    const double* q = a.q ? a.q + (size_t)b * p * n : nullptr; const double* cof = a.c ? a.c + (size_t)b * p * nx : nullptr;
    const double* D = nd > 0 ? a.D + (size_t)b * p * nd * n : nullptr; const double* dd = nd > 0 ? a.d + (size_t)b * p * nd : nullptr;
    const int* ndcnt = a.ndcnt ? a.ndcnt + (size_t)b * p : nullptr;
    auto rows_of = [&](int k) { return nd > 0 ? (ndcnt ? max(0, min(nd, ndcnt[k])) : nd) : 0; };
    const double* J = ne > 0 ? a.J + (size_t)b * p * ne * n : nullptr; const double* rq = ne > 0 && a.r ? a.r + (size_t)b * p * ne : nullptr;
    const int* necnt = a.necnt ? a.necnt + (size_t)b * p : nullptr;
    auto erows_of = [&](int k) { return ne > 0 ? (necnt ? max(0, min(ne, necnt[k])) : ne) : 0; };

    // (SOFT) c_of, z_of: penalty and penalty2 of row i of phase k (penalty absent: every row pure quadratic, c = 0; penalty2 absent: Z = 0)
    const double* pen = SOFT && a.pen ? a.pen + (size_t)b * p * nd : nullptr; const double* pen2 = SOFT && a.pen2 ? a.pen2 + (size_t)b * p * nd : nullptr;
    auto c_of = [&](int k, int i) { return pen ? pen[k * nd + i] : 0.0; };
    auto z_of = [&](int k, int i) { return pen2 ? pen2[k * nd + i] : 0.0; };
    // (SOFT) soft_at(e): entry e = j nd + i of the [N][nd] arrays is a row with two pairs; pure_at(e): a pure quadratic row (one pair); zq_at(e): its Z
    auto soft_at = [&](int e) { const int j = e / nd, i = e - j * nd, k = j % p; return i < rows_of(k) && c_of(k, i) < INFINITY && c_of(k, i) > 0.0; };
    auto pure_at = [&](int e) { const int j = e / nd, i = e - j * nd, k = j % p; return i < rows_of(k) && c_of(k, i) == 0.0; };
    auto zq_at = [&](int e) { const int j = e / nd, i = e - j * nd; return z_of(j % p, i); };

    int status = MQ_OK, its = 0;
    double mu = 0.0, rp = 0.0, rd = 0.0, pivmin = INFINITY;
    if (SOFT) {                                                              // an invalid weight: the problem ends before its first iteration
      double bad = 0.0;
      for (int e = tid; e < p * nd; e += LQR_NT) {                           // Z >= 0 and finite, 0 on a hard row; c > 0, or c = 0 with Z > 0
        const double c = c_of(e / nd, e % nd), z = z_of(e / nd, e % nd);
        if (!(z >= 0.0 && z < INFINITY) || !(c > 0.0 || (c == 0.0 && z > 0.0)) || (c == INFINITY && z != 0.0)) bad = 1.0;
      }
      if (mq_block<1>(bad, red, tid) > 0.0) status = MQ_NONFINITE;
    }
    // ---- start: z = 0 including x_0, s = max(d, 1), lam = 1, nu = 0, pi_per = 0, no direction
    int mt = 0;
    for (int j = 0; j < N; ++j) mt += rows_of(j % p);
    for (int e = tid; e < (N + 1) * n; e += LQR_NT) { Z[e] = 0.0; dZ[e] = 0.0; }
    for (int e = tid; e < N * nd; e += LQR_NT) {
      const int j = e / nd, i = e - j * nd, k = j % p;
      const bool on = i < rows_of(k);
      Sg[e] = on ? fmax(dd[k * nd + i], 1.0) : 1.0; Lg[e] = on ? 1.0 : 0.0;
      dSg[e] = 0.0; dLg[e] = 0.0; RIN[e] = 0.0; COR[e] = 0.0;
      if (SOFT) {                                                            // two pairs: lam = nu = (c + Z e) / 2, e = s; zero on the other rows (a pure row keeps lam = 1)
        const bool sf = on && c_of(k, i) < INFINITY && c_of(k, i) > 0.0;
        double hc = sf ? 0.5 * c_of(k, i) : 0.0;
        if (sf && z_of(k, i) > 0.0) { MQ_QUAD_BLOCK; hc = 0.5 * (c_of(k, i) + z_of(k, i) * Sg[e]); }
        if (sf) Lg[e] = hc;
        NUg[e] = hc; Eg[e] = sf ? Sg[e] : 0.0; dEg[e] = 0.0; C2g[e] = 0.0;
      }
    }
    for (int e = tid; e < N * ne; e += LQR_NT) { NUe[e] = 0.0; REQ[e] = 0.0; }
    for (int e = tid; e < N * nx; e += LQR_NT) PI[e] = 0.0;
    int mp = mt;                                                             // complementarity pairs: one per row, one more per row with two pairs
    if (SOFT) {
      double cnt = 0.0;
      for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) cnt += 1.0;
      mp = mt + (int)mq_block<0>(cnt, red, tid);
    }
    __syncthreads();

    for (int it = 0;; ++it) {
      its = it;
      if (SOFT) if (status != MQ_OK) break;                                  // (uniform: status is the same in every thread)
      // ================================================================== pass 1: residuals, factorisation and the border columns, j = N-1 .. 0
      if (tx < nx) for (int r = ty; r < nx; r += rs) { Pl[r * ldp + tx] = 0.0; Ml[r * ldp + tx] = r == tx ? 1.0 : 0.0; Gl[r * ldp + tx] = 0.0; }
      if (tid < nx) { const double v = PI[tid]; pip[tid] = v; pin[tid] = v; pv[tid] = v; phiv[tid] = 0.0; }
      double a_rp = 0.0, a_dyn = 0.0, a_x = 0.0, a_rd = 0.0, a_g = 0.0, a_lam = 0.0;
      int facfail = 0;
      __syncthreads();
      for (int j = N - 1; j >= 0; --j) {
        const int k = j % p, m = rows_of(k), jn = j + 1 < N ? j + 1 : 0;
        mq_fetch(El, Hl, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, H + (size_t)k * n * n, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
        if (tid < n) { zv[tid] = Z[(size_t)j * n + tid]; qv[tid] = q ? q[k * n + tid] : 0.0; }
        if (tid >= 64 && tid < 64 + nx) xn[tid - 64] = Z[(size_t)jn * n + tid - 64];
        for (int i = tid; i < m; i += LQR_NT) { lamv[i] = Lg[(size_t)j * nd + i]; sv[i] = Sg[(size_t)j * nd + i]; ddv[i] = dd[k * nd + i]; }
        if (SOFT) for (int i = tid; i < m; i += LQR_NT) { ev[i] = Eg[(size_t)j * nd + i]; nuv[i] = NUg[(size_t)j * nd + i]; cv[i] = c_of(k, i); zqv[i] = z_of(k, i); }
        const int me = erows_of(k);
        if (tx < n) for (int i = ty; i < me; i += rs) Jl[i * ld + tx] = J[((size_t)k * ne + i) * n + tx];
        for (int i = tid; i < me; i += LQR_NT) { nuev[i] = NUe[(size_t)j * ne + i]; rrv[i] = rq ? rq[k * ne + i] : 0.0; }
        __syncthreads();
        // ---- A: the residuals of the rows and of the dynamics, H z + q, Pi E
        for (int e = tid; e < m + nx + n; e += LQR_NT) {
          if (e < m) {
            const double lam = lamv[e], s = sv[e];
            double r = mq_dot(Dl + e * ld, zv, n) + s - ddv[e];
            double w = lam / (s + MQ_RHO * lam);
            double bs = w * (r + MQ_RHO * lam);
            if (SOFT) if (cv[e] < INFINITY && cv[e] > 0.0) {                 // two pairs: lam + w beta of the predictor, beta = r_in - s + e
              const double ee = ev[e];
              r = mq_dot(Dl + e * ld, zv, n) - ee + s - ddv[e];
              w = 1.0 / (s / lam + ee / nuv[e] + MQ_RHO);
              bs = lam + w * (r - s + ee);
            }
            if (SOFT) if (cv[e] < INFINITY && cv[e] > 0.0 && zqv[e] > 0.0) { // L1 + L2: nut = nu + Z e, beta = r_in - s + e nu / nut
              MQ_QUAD_BLOCK;
              const double ee = ev[e], nut = nuv[e] + zqv[e] * ee;
              w = 1.0 / (s / lam + ee / nut + MQ_RHO);
              bs = lam + w * (r - s + ee * nuv[e] / nut);
            }
            if (SOFT) if (cv[e] == 0.0) {                                    // pure quadratic: the hard row with rho + 1 / Z, r_in = D z - lam / Z + s - d
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
            if (cof) v = (mq_dot(El + r * ld, zv, n) + cof[k * nx + r]) - xn[r];
            rdynv[r] = v; RDYN[(size_t)j * nx + r] = v;
            a_dyn = cl_absmax(a_dyn, v); a_x = cl_absmax(a_x, zv[r]);
          } else {
            const int i = e - m - nx;
            gq[i] = mq_dot(Hl + i * ld, zv, n) + qv[i];
          }
        }
        for (int e = tid; e < me; e += LQR_NT) {                             // J z - r, and nu + (1 / rho)(J z - r) in the place of r
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
        // ---- B: g = H z + q + D' lam + J' nu, [pi_j; r_u] = g + E' pi_{j+1} (at j = 0 its x rows against pi_per), v = Pi r_dyn + p, Hb
        for (int e = tid; e < n + nx; e += LQR_NT) {
          if (e < n) {
            double dl = 0.0, db = 0.0, ep = 0.0;
            for (int r = 0; r < m; ++r) { const double x = Dl[r * ld + e]; dl = fma(x, lamv[r], dl); db = fma(x, bsv[r], db); }
            for (int r = 0; r < me; ++r) { const double x = Jl[r * ld + e]; dl = fma(x, nuev[r], dl); db = fma(x, rrv[r], db); }
            for (int r = 0; r < nx; ++r) ep = fma(El[r * ld + e], pin[r], ep);
            const double g = gq[e] + dl;
            a_g = cl_absmax(a_g, g);
            fullv[e] = g + ep;
            if (e >= nx) a_rd = cl_absmax(a_rd, g + ep);
            else if (j == 0) a_rd = cl_absmax(a_rd, (g + ep) - pip[e]);
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
          for (int r = 0; r < me; ++r) acc = fma(Jl[r * ld + i] * MQ_RINV, Jl[r * ld + tx], acc);
          Hl[i * ld + tx] = acc;
        }
        __syncthreads();
        // ---- C: h; its u part becomes column n of Hb; pi_j (kept in PI for j >= 1)
        if (tid < n) {
          double acc = hp[tid];
          for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + tid], vv[r], acc);
          hp[tid] = acc;
          if (tid >= nx) Hl[tid * ld + n] = acc;
          else { pin[tid] = fullv[tid]; if (j > 0) PI[(size_t)j * nx + tid] = fullv[tid]; }
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
          // ---- Pi_j = sym(Hb_xx) - Y' Y,  p_j = h_x - Y' y;  the border: T = E' M_{j+1},  phi += M_{j+1}' r_dyn
          if (tx < nx) for (int i = ty; i < nx; i += rs) {
            double acc = 0.5 * (Hl[i * ld + tx] + Hl[tx * ld + i]);
            for (int c = 0; c < mb; ++c) acc = fma(-Hl[(nx + c) * ld + i], Hl[(nx + c) * ld + tx], acc);
            Pl[i * ldp + tx] = acc;
          }
          if (tx < nx) for (int e = ty; e < n; e += rs) {
            double acc = 0.0;
            for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + e], Ml[r * ldp + tx], acc);
            Tl[e * ldp + tx] = acc;
          }
          if (tid >= 64 && tid < 64 + nx) {
            const int r = tid - 64;
            double acc = hp[r];
            for (int c = 0; c < mb; ++c) acc = fma(-Hl[(nx + c) * ld + r], Hl[(nx + c) * ld + n], acc);
            pv[r] = acc;
          }
          if (tid >= 128 && tid < 128 + nx) {
            const int c = tid - 128;
            double acc = phiv[c];
            for (int r = 0; r < nx; ++r) acc = fma(Ml[r * ldp + c], rdynv[r], acc);
            phiv[c] = acc;
          }
          __syncthreads();
          // ---- Gy_j = R^-T T_u: a thread per column, forward substitution
          if (tid < nx) for (int i = 0; i < mb; ++i) {
            double acc = Tl[(nx + i) * ldp + tid];
            for (int c = 0; c < i; ++c) acc = fma(-Hl[(nx + c) * ld + nx + i], Gyl[c * ldp + tid], acc);
            acc /= Hl[(nx + i) * ld + nx + i];
            Gyl[i * ldp + tid] = acc;
            GY[((size_t)j * mb + i) * nx + tid] = acc;
          }
          __syncthreads();
          // ---- M_j = T_x - Y' Gy_j,  Gamma += Gy_j' Gy_j,  phi -= Gy_j' y_j
          if (tx < nx) for (int r = ty; r < nx; r += rs) {
            double acc = Tl[r * ldp + tx], g = Gl[r * ldp + tx];
            for (int i = 0; i < mb; ++i) { acc = fma(-Hl[(nx + i) * ld + r], Gyl[i * ldp + tx], acc); g = fma(Gyl[i * ldp + r], Gyl[i * ldp + tx], g); }
            Ml[r * ldp + tx] = acc; Gl[r * ldp + tx] = g;
          }
          if (tid >= 128 && tid < 128 + nx) {
            const int c = tid - 128;
            double acc = phiv[c];
            for (int i = 0; i < mb; ++i) acc = fma(-Gyl[i * ldp + c], Hl[(nx + i) * ld + n], acc);
            phiv[c] = acc;
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
      rd = mq_block<1>(a_rd, red, tid) / fmax(1.0, gmax);
      mu = mt > 0 ? sumc / (SOFT ? mp : mt) : 0.0;
      if (!(rp < INFINITY && rd < INFINITY && fabs(mu) < INFINITY && lmax < INFINITY && xmax < INFINITY)) { status = MQ_NONFINITE; break; }
      if (rp <= tol && rd <= tol && mu <= MQ_MU_FACTOR * tol * fmax(1.0, lmax)) break;
      if (facfail) { status = MQ_NOT_CONVEX; break; }
      if (it == max_iter) { status = MQ_MAXITER; break; }

      // ================================================================== the border system: a, M_0 - I, R0 and W, S = Gamma + W' W = R2' R2
      if (tid < nx) av0[tid] = pv[tid] - pip[tid];
      if (tx < nx) for (int r = ty; r < nx; r += rs) if (r == tx) Ml[r * ldp + tx] -= 1.0;
      __syncthreads();
      int bfail = 0;
      for (int c = 0; c < nx; ++c) {                                         // elimination along [Pi_0 | M_0 - I], one pivot per barrier
        const double piv = Pl[c * ldp + c];
        if (!(piv > 0.0 && piv < INFINITY)) { bfail = 1; break; }
        pivmin = fmin(pivmin, piv);
        const double inv = 1.0 / piv;
        for (int i = c + 1 + ty; i < nx; i += rs) {
          const double f = Pl[c * ldp + i] * inv;
          for (int col = tx; col < 2 * nx; col += cw) {
            if (col < nx) { if (col > c) Pl[i * ldp + col] = fma(-f, Pl[c * ldp + col], Pl[i * ldp + col]); }
            else Ml[i * ldp + col - nx] = fma(-f, Ml[c * ldp + col - nx], Ml[i * ldp + col - nx]);
          }
        }
        __syncthreads();
      }
      if (!bfail) {
        if (tid < nx) dgv[tid] = 1.0 / sqrt(Pl[tid * ldp + tid]);
        __syncthreads();
        for (int i = ty; i < nx; i += rs) {
          const double sc = dgv[i];
          for (int col = tx; col < 2 * nx; col += cw) {
            if (col < nx) { if (col >= i) Pl[i * ldp + col] *= sc; }
            else Ml[i * ldp + col - nx] *= sc;
          }
        }
        __syncthreads();
        if (tx < nx) for (int r = ty; r < nx; r += rs) {
          double acc = Gl[r * ldp + tx];
          for (int i = 0; i < nx; ++i) acc = fma(Ml[i * ldp + r], Ml[i * ldp + tx], acc);
          Gl[r * ldp + tx] = acc;
        }
        __syncthreads();
        for (int c = 0; c < nx; ++c) {
          const double piv = Gl[c * ldp + c];
          if (!(piv > 0.0 && piv < INFINITY)) { bfail = 1; break; }
          pivmin = fmin(pivmin, piv);
          const double inv = 1.0 / piv;
          for (int i = c + 1 + ty; i < nx; i += rs) {
            const double f = Gl[c * ldp + i] * inv;
            for (int col = tx; col < nx; col += cw) if (col > c) Gl[i * ldp + col] = fma(-f, Gl[c * ldp + col], Gl[i * ldp + col]);
          }
          __syncthreads();
        }
      }
      if (bfail) { status = MQ_NOT_CONVEX; break; }
      if (tid < nx) dgv[tid] = 1.0 / sqrt(Gl[tid * ldp + tid]);
      __syncthreads();
      for (int i = ty; i < nx; i += rs) {
        const double sc = dgv[i];
        for (int col = tx; col < nx; col += cw) if (col >= i) Gl[i * ldp + col] *= sc;
      }
      __syncthreads();
      border_solve(av0, phiv);

      double alpha = 1.0;
      for (int sweep = 0; sweep < 2; ++sweep) {
        if (sweep == 1) {
          if (mt == 0) break;
          // ================================================================ the corrector: sigma, c, and the change of y swept backward
          const double aa = fmin(1.0, alpha);
          part = 0.0;
          for (int e = tid; e < N * nd; e += LQR_NT) part = fma(Lg[e] + aa * dLg[e], Sg[e] + aa * dSg[e], part);
          if (SOFT) for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) {
            if (zq_at(e) > 0.0) { MQ_QUAD_BLOCK; part = fma(Eg[e] + aa * dEg[e], NUg[e] + aa * (zq_at(e) * dEg[e] - dLg[e]), part); }      // dnu = Z de - dlam
            else part = fma(Eg[e] + aa * dEg[e], NUg[e] - aa * dLg[e], part);
          }
          const double r3 = mq_block<0>(part, red, tid) / (SOFT ? mp : mt) / mu;
          const double sigmu = r3 * r3 * r3 * mu;
          for (int e = tid; e < N * nd; e += LQR_NT) {
            const int j = e / nd, i = e - j * nd;
            COR[e] = i < rows_of(j % p) ? (sigmu - dSg[e] * dLg[e]) / (Sg[e] + MQ_RHO * Lg[e]) : 0.0;
            if (SOFT) if (soft_at(e)) {                                      // w (c1 / lam - c2 / nu), and c2 / nu (C2) for the forward sweep
              double c2 = (sigmu + dEg[e] * dLg[e]) / NUg[e];
              COR[e] = ((sigmu - dSg[e] * dLg[e]) / Lg[e] - c2) / (Sg[e] / Lg[e] + Eg[e] / NUg[e] + MQ_RHO);
              if (zq_at(e) > 0.0) {                                          // c2 = sigma mu - de_aff dnu_aff, over nut
                MQ_QUAD_BLOCK;
                const double z = zq_at(e), nut = NUg[e] + z * Eg[e];
                c2 = (sigmu - dEg[e] * (z * dEg[e] - dLg[e])) / nut;
                COR[e] = ((sigmu - dSg[e] * dLg[e]) / Lg[e] - c2) / (Sg[e] / Lg[e] + Eg[e] / nut + MQ_RHO);
              }
              C2g[e] = c2;
            }
            if (SOFT) if (pure_at(e)) { MQ_QUAD_BLOCK; COR[e] = (sigmu - dSg[e] * dLg[e]) / (Sg[e] + (MQ_RHO + 1.0 / zq_at(e)) * Lg[e]); }
          }
          if (tid < nx) { dxa[tid] = 0.0; phic[tid] = phiv[tid]; }           // dp_N = 0: dpi is carried by the border columns
          __syncthreads();
          double* dp = dxa; double* dpn = dxb;
          for (int j = N - 1; j >= 0; --j) {
            const int k = j % p, m = rows_of(k);
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
            if (wave == 0) {                                                 // R' dy = dh_u, column by column inside one wave
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
            if (tid >= 64 && tid < 64 + nx) {                                // dphi -= Gy_j' dy_j
              const int c = tid - 64;
              double acc = phic[c];
              for (int i = 0; i < mb; ++i) acc = fma(-GY[((size_t)j * mb + i) * nx + c], dyv[i], acc);
              phic[c] = acc;
            }
            __syncthreads();
            { double* t_ = dp; dp = dpn; dpn = t_; }
          }
          if (tid < nx) av1[tid] = av0[tid] + dp[tid];
          __syncthreads();
          border_solve(av1, phic);
        }
        // ================================================================== the forward sweep from dx_0: the direction and its largest step
        if (tid < nx) dxa[tid] = dx0[tid];
        __syncthreads();
        double* dx = dxa; double* dxn = dxb;
        double amin = 1e300;
        const bool last = sweep == 1 || mt == 0;                             // the sweep whose direction is taken: it computes dnu
        for (int j = 0; j < N; ++j) {
          const int k = j % p, m = rows_of(k);
          const int me = last ? erows_of(k) : 0;
          if (last) {
            if (tx < n) for (int i = ty; i < me; i += rs) Jl[i * ld + tx] = J[((size_t)k * ne + i) * n + tx];
            for (int i = tid; i < me; i += LQR_NT) reqv[i] = REQ[(size_t)j * ne + i];
          }
          mq_fetch(El, nullptr, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, nullptr, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
          for (int i = ty; i < mb; i += rs) for (int col = tx; col <= n; col += cw) Hl[(nx + i) * ld + col] = FAC[(size_t)j * fs + i * (n + 1) + col];
          for (int i = tid; i < m; i += LQR_NT) {
            lamv[i] = Lg[(size_t)j * nd + i]; sv[i] = Sg[(size_t)j * nd + i]; rinv[i] = RIN[(size_t)j * nd + i]; corv[i] = sweep ? COR[(size_t)j * nd + i] : 0.0;
          }
          if (SOFT) for (int i = tid; i < m; i += LQR_NT) { ev[i] = Eg[(size_t)j * nd + i]; nuv[i] = NUg[(size_t)j * nd + i]; cv[i] = c_of(k, i); zqv[i] = z_of(k, i); }
          if (tid >= 64 && tid < 64 + nx) rdynv[tid - 64] = RDYN[(size_t)j * nx + tid - 64];
          __syncthreads();
          if (wave == 0) {                                                   // du = -R^-1 (Y dx + y + Gy dpi), column by column inside one wave
            double tt = lane < mb ? (mq_dot(Hl + (nx + lane) * ld, dx, nx) + Hl[(nx + lane) * ld + n]) + mq_dot(GY + ((size_t)j * mb + lane) * nx, dpi, nx) : 0.0;
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
              if (SOFT) if (cv[e] < INFINITY && cv[e] > 0.0 && !(zqv[e] > 0.0)) {      // L1: de = -e + c2 / nu + (e / nu) dlam, dnu = -dlam
                const double ee = ev[e], nu = nuv[e];
                const double ws_ = 1.0 / (s / lam + ee / nu + MQ_RHO);
                dl = corv[e] + ws_ * (rinv[e] - s + ee + Dz);
                const double de = -ee + (sweep ? C2g[(size_t)j * nd + e] : 0.0) + (ee / nu) * dl;
                ds = -rinv[e] - Dz + de + MQ_RHO * dl;
                dEg[(size_t)j * nd + e] = de;
                if (de < 0.0) amin = fmin(amin, -ee / de);
                if (dl > 0.0) amin = fmin(amin, nu / dl);
              }
              if (SOFT) if (cv[e] < INFINITY && cv[e] > 0.0 && zqv[e] > 0.0) {         // L1 + L2: de = (c2 - e nu + e dlam) / nut, dnu = Z de - dlam
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
              if (SOFT) if (cv[e] == 0.0) {                                  // pure quadratic: the hard row with rho + 1 / Z
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
          for (int e = tid; e < me; e += LQR_NT) REQ[(size_t)j * ne + e] = MQ_RINV * (mq_dot(Jl + e * ld, dzv, n) + reqv[e]);     // dnu
          __syncthreads();
          { double* t_ = dx; dx = dxn; dxn = t_; }
        }
        alpha = mq_block<2>(amin, red, tid);
      }
      // ==================================================================== the step
      const double al = fmin(1.0, MQ_STEP_BACK * alpha);
      for (int e = tid; e < N * n; e += LQR_NT) Z[e] = fma(al, dZ[e], Z[e]);
      if (SOFT) for (int e = tid; e < N * nd; e += LQR_NT) if (soft_at(e)) {
        if (zq_at(e) > 0.0) { MQ_QUAD_BLOCK; NUg[e] = fma(al, zq_at(e) * dEg[e] - dLg[e], NUg[e]); Eg[e] = fma(al, dEg[e], Eg[e]); }
        else { Eg[e] = fma(al, dEg[e], Eg[e]); NUg[e] = fma(-al, dLg[e], NUg[e]); }
      }
      for (int e = tid; e < N * nd; e += LQR_NT) { Sg[e] = fma(al, dSg[e], Sg[e]); Lg[e] = fma(al, dLg[e], Lg[e]); }
      for (int e = tid; e < N * ne; e += LQR_NT) NUe[e] = fma(al, REQ[e], NUe[e]);
      if (tid < nx) PI[tid] = fma(al, dpi[tid], PI[tid]);
      __syncthreads();
    }

    // ---- the results: the orbit, the multipliers (Pi[0] = pi_per, Pi[j] the adjoint of the last pass 1), cost, hres, eres, per
    __syncthreads();
    const bool ok = status == MQ_OK;
    double cost = qnan, hres = qnan, eres = qnan, per = qnan;
    double pcost = qnan, emax = qnan;                                        // (SOFT)
    int nviol = -1;                                                          // (SOFT)
    if (ok) {
      double csum = 0.0, hmax = -INFINITY, em = 0.0, pm = 0.0;
      for (int j = 0; j < N; ++j) {
        const int k = j % p, m = rows_of(k), me = erows_of(k);
        mq_fetch(El, Hl, Dl, ld, A + (size_t)k * nx * nx, B + (size_t)k * nx * mb, H + (size_t)k * n * n, D ? D + (size_t)k * nd * n : nullptr, nx, mb, m, tx, ty, rs);
        if (tx < n) for (int i = ty; i < me; i += rs) Jl[i * ld + tx] = J[((size_t)k * ne + i) * n + tx];
        if (tid < n) zv[tid] = Z[(size_t)j * n + tid];
        if (tid >= 64 && tid < 64 + nx) xn[tid - 64] = Z[tid - 64];
        __syncthreads();
        if (tid < n) csum += zv[tid] * (0.5 * mq_dot(Hl + tid * ld, zv, n) + (q ? q[k * n + tid] : 0.0));
        for (int i = tid; i < m; i += LQR_NT) hmax = fmax(hmax, mq_dot(Dl + i * ld, zv, n) - dd[k * nd + i]);
        for (int i = tid; i < me; i += LQR_NT) em = cl_absmax(em, mq_dot(Jl + i * ld, zv, n) - (rq ? rq[k * ne + i] : 0.0));
        if (j == N - 1 && tid < nx) pm = cl_absmax(pm, (mq_dot(El + tid * ld, zv, n) + (cof ? cof[k * nx + tid] : 0.0)) - xn[tid]);
        __syncthreads();
      }
      cost = mq_block<0>(csum, red, tid); hres = mq_block<1>(hmax, red, tid); eres = mq_block<1>(em, red, tid); per = mq_block<1>(pm, red, tid);
      if (SOFT) {                                                            // the slacks: e (lam / Z on a pure row), their cost c e + 1/2 Z e^2, the violated rows
        double pc = 0.0, emx = 0.0, cnt = 0.0;
        for (int e = tid; e < N * nd; e += LQR_NT) {
          const int j = e / nd, i = e - j * nd, k = j % p;
          double ee = 0.0;
          if (soft_at(e)) { ee = Eg[e]; if (Eg[e] > NUg[e]) cnt += 1.0; }
          if (pure_at(e)) { ee = Lg[e] / z_of(k, i); if (Lg[e] > Sg[e]) cnt += 1.0; }
          if (soft_at(e) || pure_at(e)) pc += c_of(k, i) * ee + 0.5 * z_of(k, i) * ee * ee;
          emx = fmax(emx, ee);
          if (a.Eps) a.Eps[(size_t)b * N * nd + e] = ee;
        }
        pcost = mq_block<0>(pc, red, tid); emax = mq_block<1>(emx, red, tid); nviol = (int)mq_block<0>(cnt, red, tid);
        cost = cost + pcost;
      }
    }
    if (SOFT) if (!ok) if (a.Eps) for (int e = tid; e < N * nd; e += LQR_NT) a.Eps[(size_t)b * N * nd + e] = qnan;
    const size_t bb = (size_t)b;
    if (a.X) for (int e = tid; e < N * nx; e += LQR_NT) { const int j = e / nx; a.X[bb * N * nx + e] = ok ? Z[(size_t)j * n + e - j * nx] : qnan; }
    if (a.U) for (int e = tid; e < N * mb; e += LQR_NT) { const int j = e / mb; a.U[bb * N * mb + e] = ok ? Z[(size_t)j * n + nx + e - j * mb] : qnan; }
    if (a.Lam) for (int e = tid; e < N * nd; e += LQR_NT) a.Lam[bb * N * nd + e] = ok ? Lg[e] : qnan;
    if (a.Nu) for (int e = tid; e < N * ne; e += LQR_NT) a.Nu[bb * N * ne + e] = ok ? NUe[e] : qnan;
    if (a.Pi) for (int e = tid; e < N * nx; e += LQR_NT) a.Pi[bb * N * nx + e] = ok ? PI[e] : qnan;
    if (tid == 0) {
      double* o = a.info + bb * PQ_INFO;
      o[0] = status; o[1] = ok ? 1.0 : 0.0; o[2] = its; o[3] = its; o[4] = mu; o[5] = rp; o[6] = rd; o[7] = pivmin;
      if (!SOFT) if (a.res) { double* r = a.res + bb * PQ_RES; r[0] = cost; r[1] = hres; r[2] = eres; r[3] = per; }
      if (SOFT) {
        if (a.res) { double* r = a.res + bb * PQ_RES_SOFT; r[0] = cost; r[1] = hres; r[2] = eres; r[3] = per; r[4] = pcost; r[5] = emax; }
        if (a.nviol) a.nviol[bb] = nviol;
      }
    }
    __syncthreads();
  }
}

}  // namespace tmpc
