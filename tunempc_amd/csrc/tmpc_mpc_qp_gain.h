// The local feedback gain of a solved inequality-constrained MPC step (tmpc_mpc_qp.h): at a strictly complementary solution the QP is locally piecewise
// affine in x_0, u_0(x_0 + dx) = u_0 - K_0 dx, and K_0 is the first gain of the equality-constrained LQ problem that keeps the current active set.  Every row
// (j, i) of the horizon falls into one class, decided by the solver's own activity rules (nact: lam > s; nviol: e > nu) with g = d_i - D_i z_j:
//   hard row (c = inf)                 s = g                                      1 if lam > s, else 0
//   pure quadratic (c = 0, Z > 0)      s = g + lam / Z                            2 if lam > s, else 0
//   L1 and L1 + L2 (0 < c < inf)       s = g + e,  nu = c + Z e - lam             0 if not lam > s; else violated (e > nu): 2 if Z > 0, 0 if Z = 0; else 1
//   rows beyond ndcnt                                                             0
// (c = 0 with Z = 0, which the Python layer refuses, is class 0 with s = g: nothing is divided by zero.)
// class 0 (free): the row drops out; class 1 (equality): D_i dz_j = 0; class 2 (quadratic): the stage Hessian gains Z_i D_i' D_i.  The equality rows J_k and
// the terminal rows always hold.  q, r, offset, qf and terminal_rhs enter only through the solution and are no arguments.  cls_in replaces the rule (values
// other than 1 and 2 count as 0): the gain at any active set.
//
// The recursion is the constraint-to-go stage of k_horizon_lqr (tmpc_lqr_ctg.h, steps 1-5) on a copy that lives here, so that the LQR kernels and the QP kernel
// stay as they are.  The stack of a stage is [J_k rows; class-1 rows of D_k in ascending i; Hn_{j+1} E], its Hessian (H_k + H_k') / 2 + sum_class2 Z_i D_i' D_i
// (ascending i), and the pass starts from Pi_N = (Pf + Pf') / 2 with Hn_N empty (terminal 0), the identity (1: x_N = 0) or the rows of Tx orthonormalised by
// the compression of step 3 (2; all nx directions may be taken at that given stage only).  No row enters at a penalty weight: the gain is exact at the active
// set, more active rows than inputs, rows on the state alone and dependent rows included; K0, Pi0 come out projected on Hn0 dx = 0, the directions in which
// the active set can be kept.
//
// Residency: grid (ns, nb), one 256-thread workgroup per (problem, instance), one backward pass j = N-1 ... 0 over k = (k0 + j) mod p, the LDS layout of
// lqr_ctg_lds(nx, mb, ne + nd) followed by 2 nd + 2 ints (class and stack position per row, the two counts).  Per stage the rows are classified from X_j, U_j,
// Lam_j, Eps_j, d, penalty, penalty2 in global memory, one row per thread with a serial dot product; thread 0 numbers the class-1 rows; every decision after
// that is taken on values all threads read from LDS, every sum runs in a fixed order: the numbers of an instance do not depend on ns, on its neighbours or on
// the grid.  fp64 on the vector ALU.
//
// strict = min over every complementarity pair (lam, s) and, on two-pair rows, (e, nu) of |a - b| / max(|a|, |b|): near 1 when the active set is unambiguous,
// near 0 on a weakly active row, where the derivative is one-sided and the result means nothing.  With dX the forward pass of the same launch writes the
// open-loop sensitivities Phi_0 = Pz_0, dU_j = -K_j Phi_j, Phi_{j+1} = (A - B K_j) Phi_j (K_j read back from Kall).
//
// Statuses as in k_horizon_lqr: 0 done, 2 singular stage system, 3 non-finite, 5 no feasible subspace.  An instance whose X, U, Lam or Eps hold a non-finite
// entry (a failed solve returns NaN) ends with status 3 before its first stage.  status >= 2: K0, Pi0, strict, dX, dU NaN, Hn0 zero, cnt0 the count of the
// failing stage, and NaN / -1 in the stages of Kall / cntall / cls that were not finished.  Not served: multiplier sensitivities.
#pragma once
#include "tmpc_lqr_ctg.h"

namespace tmpc {

enum { MQG_TERMINAL_NONE = 0, MQG_TERMINAL_ORIGIN = 1, MQG_TERMINAL_ROWS = 2 };

__host__ __device__ inline int mpc_qp_gain_lds_doubles(int nx, int mb, int ne, int nd) { return lqr_ctg_lds(nx, mb, ne + nd).total + nd + 1; }

// A [nb][p][nx][nx], B [nb][p][nx][mb], H [nb][p][n][n], Pf [nb][p][nx][nx] or null, D [nb][p][nd][n], ndcnt [nb][p] or null, d, pen, pen2 [nb][p][nd] (pen
// null: all hard; pen2 null: zero), J [nb][p][ne][n], necnt [nb][p] or null, Tx [nb][p][nt][nx]; the solution X [nb][ns][N+1][nx], U [nb][ns][N][mb],
// Lam, Eps [nb][ns][N][nd] (Eps null: zero); cls_in int [nb][ns][N][nd] or null.
// Outputs: K0 [nb][ns][mb][nx], Pi0, Hn0 [nb][ns][nx][nx], cnt0 [nb][ns], info [nb][ns][12]; each or null: cls int [nb][ns][N][nd], strict [nb][ns],
// Kall [nb][ns][N][mb][nx], cntall [nb][ns][N], dX [nb][ns][N+1][nx][nx], dU [nb][ns][N][mb][nx] (dX, dU together and with Kall).
struct MpcQpGainArgs {
  int p, nx, mb, nd, ne, nt, N, k0, terminal, lcw;
  const double *A, *B, *H, *Pf, *D, *d, *pen, *pen2, *J, *Tx, *X, *U, *Lam, *Eps;
  const int *ndcnt, *necnt, *cls_in;
  double rank_tol;
  double *K0, *Pi0, *Hn0;
  int* cnt0;
  double* info;
  int* cls;
  double *strict, *Kall;
  int* cntall;
  double *dX, *dU;
};

__device__ __forceinline__ double mqg_pair(double a, double b) {             // strictness of one complementarity pair
  const double m = fmax(fabs(a), fabs(b));
  return m > 0.0 ? fabs(a - b) / m : 0.0;
}

__global__ void __launch_bounds__(LQR_NT) k_mpc_qp_gain(const MpcQpGainArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int p = a.p, nx = a.nx, mb = a.mb, nd = a.nd, ne = a.ne, nt = a.nt, N = a.N, lcw = a.lcw;
  const int n = nx + mb;
  const LqrCtgLds L = lqr_ctg_lds(nx, mb, ne + nd);
  const int ld = L.ld, ldp = L.ldp, ldc = L.ldc, nbd = L.nbd;
  double* El = lds + L.oE; double* Pl = lds + L.oP; double* Wl = lds + L.oW; double* Hl = lds + L.oH; double* red = lds + L.oR;
  double* C0 = lds + L.oC0; double* C1 = lds + L.oC1; double* HnN = lds + L.oN0; double* HnC = lds + L.oN1;
  int* clsl = (int*)(lds + L.total); int* posl = clsl + nd; int* cntl = posl + nd;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const size_t si = blockIdx.x, ns = gridDim.x, b = blockIdx.y, bi = b * ns + si;
  const int k0 = a.k0, kN = (k0 + N % p) % p;
  const double* A = a.A + b * p * nx * nx; const double* B = a.B + b * p * nx * mb; const double* H = a.H + b * p * n * n;
  const double* D = nd > 0 ? a.D + b * p * nd * n : nullptr; const double* dd = nd > 0 ? a.d + b * p * nd : nullptr;
  const double* pen = (nd > 0 && a.pen) ? a.pen + b * p * nd : nullptr; const double* pen2 = (nd > 0 && a.pen2) ? a.pen2 + b * p * nd : nullptr;
  const double* J = ne > 0 ? a.J + b * p * ne * n : nullptr;
  const int* ndcnt = a.ndcnt ? a.ndcnt + b * p : nullptr; const int* necnt = a.necnt ? a.necnt + b * p : nullptr;
  const double* X = a.X + bi * (N + 1) * nx; const double* U = a.U + bi * N * mb;
  const double* Lam = nd > 0 ? a.Lam + bi * N * nd : nullptr; const double* Eps = (nd > 0 && a.Eps) ? a.Eps + bi * N * nd : nullptr;
  const int* cls_in = (nd > 0 && a.cls_in) ? a.cls_in + bi * N * nd : nullptr;
  double* K0 = a.K0 + bi * mb * nx; double* Pi0 = a.Pi0 + bi * nx * nx; double* Hn0 = a.Hn0 + bi * nx * nx;
  double* Kall = a.Kall ? a.Kall + bi * N * mb * nx : nullptr; int* cntall = a.cntall ? a.cntall + bi * N : nullptr;
  int* clso = (nd > 0 && a.cls) ? a.cls + bi * N * nd : nullptr;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  auto rows_of = [&](int k) { return ndcnt ? max(0, min(nd, ndcnt[k])) : nd; };
  auto erows_of = [&](int k) { return necnt ? max(0, min(ne, necnt[k])) : ne; };

  // ---- a solution with a non-finite entry is no solution: status 3 before the first stage
  double bad0 = 0.0;
  for (int e = tid; e < (N + 1) * nx; e += LQR_NT) if (!(fabs(X[e]) < INFINITY)) bad0 = 1.0;
  for (int e = tid; e < N * mb; e += LQR_NT) if (!(fabs(U[e]) < INFINITY)) bad0 = 1.0;
  for (int e = tid; e < N * nd; e += LQR_NT) {
    const int j = e / nd, i = e - j * nd;
    if (i < rows_of((k0 + j % p) % p)) {
      if (!(fabs(Lam[e]) < INFINITY)) bad0 = 1.0;
      if (Eps) if (!(fabs(Eps[e]) < INFINITY)) bad0 = 1.0;
    }
  }
  bad0 = lqr_wave_max(bad0);
  if (lane == 0) red[4 + wv] = bad0;
  __syncthreads();
  bad0 = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));

  int status = bad0 > 0.0 ? LQR_NONFINITE : LQR_OK, done = 0, csum = 0, cmax = 0, cfail = 0;
  double pmin = INFINITY, pmax = 0.0, posdef = 1.0, accmin = INFINITY, rejmax = 0.0, feas = 0.0, strict = INFINITY;

  // ---- the start of the pass: Pi_N and Hn_N
  int cn = a.terminal == MQG_TERMINAL_ORIGIN ? nx : 0;
  if (tx < nx) {
    const double* Pn = a.Pf ? a.Pf + (b * p + (size_t)kN) * nx * nx : nullptr;
    for (int r = ty; r < nx; r += rs) {
      Pl[r * ldp + tx] = Pn ? 0.5 * (Pn[r * nx + tx] + Pn[tx * nx + r]) : 0.0;
      if (cn) HnN[r * ldp + tx] = (r == tx) ? 1.0 : 0.0;
    }
  }
  if (a.terminal == MQG_TERMINAL_ROWS && status == LQR_OK) {                 // the rows of Tx through the compression of a stage, into Hn_N
    const double* Tx = a.Tx + (b * p + (size_t)kN) * nt * nx;
    if (tx < nx) for (int i = ty; i < nt; i += rs) C0[i * ldc + tx] = Tx[i * nx + tx];
    __syncthreads();
    double* cs = C0; double* cd = C1;
    double v = 0.0;
    for (int q = lane; q < nt * nx; q += 64) {
      const int i = q / nx;
      double x = fabs(cs[i * ldc + q - i * nx]);
      if (x != x) x = INFINITY;
      v = fmax(v, x);
    }
    const double scale = fmax(1.0, lqr_wave_max(v));
    if (!(scale < INFINITY)) status = LQR_NONFINITE;
    const double thr = a.rank_tol * scale;
    int c = 0;
    while (status == LQR_OK) {
      const int rem = nt - c;
      if (rem <= 0) break;
      double vb = -1.0; int vi = 0;
      for (int q = lane; q < rem; q += 64) {
        double s2 = 0.0;
        for (int s = 0; s < nx; ++s) { const double x = cs[(c + q) * ldc + s]; s2 = fma(x, x, s2); }
        if (s2 != s2) s2 = INFINITY;
        if (s2 > vb) { vb = s2; vi = q; }
      }
      const double vmax = lqr_wave_max(vb), nrm = sqrt(vmax);
      if (!(nrm > thr)) { rejmax = fmax(rejmax, nrm / scale); break; }
      const int pr = c + lqr_wave_min(vb == vmax ? vi : 0x7fffffff);
      accmin = fmin(accmin, nrm / scale);
      const double inv = 1.0 / nrm, inv2 = 1.0 / vmax;
      if (tx < nx) {
        const double prow = cs[pr * ldc + tx];
        if (ty == 0) HnN[c * ldp + tx] = prow * inv;
        for (int i = c + 1 + ty; i < nt; i += rs) {
          const int q = (i == pr) ? c : i;
          double dot = 0.0;
          for (int s = 0; s < nx; ++s) dot = fma(cs[q * ldc + s], cs[pr * ldc + s], dot);
          cd[i * ldc + tx] = fma(-dot * inv2, prow, cs[q * ldc + tx]);
        }
      }
      __syncthreads();
      double* t_ = cs; cs = cd; cd = t_;
      ++c;
    }
    cn = c; cfail = c;
  }
  __syncthreads();

  for (int j = status == LQR_OK ? N - 1 : -1; j >= 0; --j) {
    const int k = (k0 + j % p) % p;
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Hk = H + (size_t)k * n * n;
    const double* Jk = J ? J + (size_t)k * ne * n : nullptr; const double* Dk = D ? D + (size_t)k * nd * n : nullptr;
    const int md = rows_of(k), me = erows_of(k);
    // ---- the class of every row of D_k, one row per thread
    {
      const double* Xj = X + (size_t)j * nx; const double* Uj = U + (size_t)j * mb;
      for (int i = tid; i < nd; i += LQR_NT) {
        int c_ = 0;
        if (i < md) {
          const double* Di = Dk + (size_t)i * n;
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(Di[s], Xj[s], acc);
          for (int s = 0; s < mb; ++s) acc = fma(Di[nx + s], Uj[s], acc);
          const double g = dd[k * nd + i] - acc, lam = Lam[(size_t)j * nd + i], e = Eps ? Eps[(size_t)j * nd + i] : 0.0;
          const double cp = pen ? pen[k * nd + i] : INFINITY, Z = pen2 ? pen2[k * nd + i] : 0.0;
          if (cp == INFINITY) {
            strict = fmin(strict, mqg_pair(lam, g));
            c_ = lam > g ? 1 : 0;
          } else if (cp == 0.0) {
            const double s = Z > 0.0 ? g + lam / Z : g;                        // (c = 0 with Z = 0 is no row kind: taken as a row that cannot be active)
            strict = fmin(strict, mqg_pair(lam, s));
            c_ = (lam > s && Z > 0.0) ? 2 : 0;
          } else {
            const double s = g + e, nu = cp + Z * e - lam;
            strict = fmin(strict, fmin(mqg_pair(lam, s), mqg_pair(e, nu)));
            if (lam > s) c_ = e > nu ? (Z > 0.0 ? 2 : 0) : 1;
          }
          if (cls_in) { c_ = cls_in[(size_t)j * nd + i]; if ((c_ != 1 && c_ != 2) || (c_ == 2 && !(Z > 0.0))) c_ = 0; }
        }
        clsl[i] = c_;
        if (clso) clso[(size_t)j * nd + i] = c_;
      }
    }
    __syncthreads();
    if (tid == 0) {                                                          // the class-1 rows take their places in the stack in ascending i
      int n1 = 0, n2 = 0;
      for (int i = 0; i < md; ++i) { posl[i] = n1; if (clsl[i] == 1) ++n1; else if (clsl[i] == 2) ++n2; }
      cntl[0] = n1; cntl[1] = n2;
    }
    __syncthreads();
    const int rk = me + cntl[0], n2 = cntl[1];
    // ---- operands of the stage (Pi_{j+1}, Hn_{j+1} stand where the last stage left them)
    if (tx < n) {
      for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
      for (int r = ty; r < n; r += rs) {
        double acc = 0.5 * (Hk[r * n + tx] + Hk[tx * n + r]);
        if (n2 > 0) for (int i = 0; i < md; ++i) if (clsl[i] == 2) acc = fma(pen2[k * nd + i] * Dk[i * n + r], Dk[i * n + tx], acc);
        Hl[r * ld + tx] = acc;
      }
      for (int i = ty; i < me; i += rs) C0[i * ldc + tx] = Jk[i * n + tx];
      for (int i = ty; i < md; i += rs) if (clsl[i] == 1) C0[(me + posl[i]) * ldc + tx] = Dk[i * n + tx];
    }
    if (tx < nbd) for (int i = ty; i < nbd; i += rs) Hl[(n + i) * ld + n + tx] = 0.0;
    __syncthreads();
    // ---- W = Pi_{j+1} E; the constraint-to-go seen from this stage, Hn_{j+1} E, below the rows of the stage
    if (tx < n) {
      for (int r = ty; r < nx; r += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(Pl[r * ldp + s], El[s * ld + tx], acc);
        Wl[r * ld + tx] = acc;
      }
      for (int i = ty; i < cn; i += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(HnN[i * ldp + s], El[s * ld + tx], acc);
        C0[(rk + i) * ldc + tx] = acc;
      }
    }
    __syncthreads();
    // ---- Hb = H_k + sum_class2 Z D'D + E' W
    if (tx < n) for (int i = ty; i < n; i += rs) {
      double acc = Hl[i * ld + tx];
      for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + i], Wl[r * ld + tx], acc);
      Hl[i * ld + tx] = acc;
    }
    __syncthreads();
    // ---- split and compress: cs -> cd, one pivot per barrier
    const int m = rk + cn;
    int rho = 0, c = 0;
    double* cs = C0; double* cd = C1;
    if (m > 0) {
      double v = 0.0;
      for (int q = lane; q < m * n; q += 64) {
        const int i = q / n;
        double x = fabs(cs[i * ldc + q - i * n]);
        if (x != x) x = INFINITY;
        v = fmax(v, x);
      }
      const double scale = fmax(1.0, lqr_wave_max(v));
      if (!(scale < INFINITY)) { status = LQR_NONFINITE; break; }
      const double thr = a.rank_tol * scale;
      double sfac = (lane < mb) ? fabs(Hl[(nx + lane) * ld + nx + lane]) : 0.0;      // the scale of S: its largest diagonal entry
      sfac = lqr_wave_max(sfac);
      if (!(sfac > 0.0 && sfac < INFINITY)) sfac = 1.0;
      for (;;) {                                                           // the split: full pivoting on the Cu block of the rows rho .. m-1
        const int rem = m - rho;
        if (rem == 0) break;
        double vb = -1.0; int vi = 0;
        for (int q = lane; q < rem * mb; q += 64) {
          const int i = q / mb;
          const double x = fabs(cs[(rho + i) * ldc + nx + q - i * mb]);
          if (x > vb) { vb = x; vi = q; }
        }
        const double vmax = lqr_wave_max(vb);
        if (rho == nbd || !(vmax > thr)) { rejmax = fmax(rejmax, vmax / scale); break; }
        const int qi = lqr_wave_min(vb == vmax ? vi : 0x7fffffff);           // the first entry that holds the maximum
        accmin = fmin(accmin, vmax / scale);
        const int pr = rho + qi / mb, pc = nx + qi % mb;
        const double inv = 1.0 / cs[pr * ldc + pc];
        if (tx < n) {
          const double prow = cs[pr * ldc + tx];
          if (ty == 0) { const double br = prow * (sfac / vmax); Hl[(n + rho) * ld + tx] = br; Hl[tx * ld + n + rho] = br; }      // final: into the border, pivot scaled to S
          for (int i = rho + 1 + ty; i < m; i += rs) {
            const int q = (i == pr) ? rho : i;                             // row pr receives what stood in row rho
            const double f = cs[q * ldc + pc] * inv;
            cd[i * ldc + tx] = (tx == pc) ? 0.0 : fma(-f, prow, cs[q * ldc + tx]);
          }
        }
        __syncthreads();
        double* t_ = cs; cs = cd; cd = t_;
        ++rho;
      }
      for (;;) {                                                           // the compression: Gram-Schmidt on the x parts of the rows rho + c .. m-1
        const int base = rho + c, rem = m - base;
        if (rem <= 0) break;
        double vb = -1.0; int vi = 0;
        for (int q = lane; q < rem; q += 64) {
          double s2 = 0.0;
          for (int s = 0; s < nx; ++s) { const double x = cs[(base + q) * ldc + s]; s2 = fma(x, x, s2); }
          if (s2 != s2) s2 = INFINITY;
          if (s2 > vb) { vb = s2; vi = q; }
        }
        const double vmax = lqr_wave_max(vb), nrm = sqrt(vmax);
        if (!(nrm > thr)) { rejmax = fmax(rejmax, nrm / scale); break; }
        const int pr = base + lqr_wave_min(vb == vmax ? vi : 0x7fffffff);
        accmin = fmin(accmin, nrm / scale);
        if (c + 1 == nx) { status = LQR_NO_FEASIBLE; c = nx; break; }       // x_j = 0 is all that is left
        const double inv = 1.0 / nrm, inv2 = 1.0 / vmax;
        if (tx < nx) {
          const double prow = cs[pr * ldc + tx];
          if (ty == 0) HnC[c * ldp + tx] = prow * inv;
          for (int i = base + 1 + ty; i < m; i += rs) {
            const int q = (i == pr) ? base : i;
            double dot = 0.0;
            for (int s = 0; s < nx; ++s) dot = fma(cs[q * ldc + s], cs[pr * ldc + s], dot);
            cd[i * ldc + tx] = fma(-dot * inv2, prow, cs[q * ldc + tx]);
          }
        }
        __syncthreads();
        double* t_ = cs; cs = cd; cd = t_;
        ++c;
      }
    }
    cfail = c;
    if (status != LQR_OK) break;
    const int nk = mb + rho, wid = n + rho;
    // ---- [M; Jx~ | S Ju~'; Ju~ 0] -> [K; Lam | I]: one pivot per barrier, src -> dst
    double* src = Hl + nx * ld; double* dst = Wl;
    double spmax = 0.0;
    for (int cc = 0; cc < nk; ++cc) {
      const int pc = nx + cc, rem = nk - cc;
      double v = -1.0; int vi = 0;
      for (int q = lane; q < rem; q += 64) {
        double x = fabs(src[(cc + q) * ld + pc]);
        if (x != x) x = INFINITY;
        if (x > v) { v = x; vi = q; }
      }
      const double vmax = lqr_wave_max(v);
      int pr;
      if (rem <= 64) pr = cc + __ffsll((long long)__ballot(v == vmax)) - 1;
      else pr = cc + lqr_wave_min(v == vmax ? vi : 0x7fffffff);
      const double diag = src[cc * ld + pc];
      const bool keep = cc < mb ? (diag > 0.0 && diag >= LQR_PIV_THRESH * vmax) : (diag < 0.0 && -diag >= LQR_PIV_THRESH * vmax);
      if (keep) pr = cc; else posdef = 0.0;
      const double pv = src[pr * ld + pc], apv = fabs(pv);
      if (!(apv < INFINITY)) { status = LQR_NONFINITE; break; }
      if (!(apv > LQR_SING_REL * spmax)) { status = LQR_SINGULAR; pmin = fmin(pmin, apv); break; }
      spmax = fmax(spmax, apv); pmin = fmin(pmin, apv); pmax = fmax(pmax, apv);
      const double inv = 1.0 / pv;
      for (int col = tx; col < wid; col += cw) {
        if (col >= nx && col <= pc) continue;
        const double pj = src[pr * ld + col] * inv;
        for (int r = ty; r < nk; r += rs) {
          const int q = (r == pr) ? cc : r;
          dst[r * ld + col] = (r == cc) ? pj : fma(-src[q * ld + pc], pj, src[q * ld + col]);
        }
      }
      __syncthreads();
      double* t_ = src; src = dst; dst = t_;
    }
    if (status != LQR_OK) break;
    // ---- Hb_xx - [M; Jx~]' [K; Lam]
    if (tx < nx) for (int i = ty; i < nx; i += rs) {
      double acc = Hl[i * ld + tx];
      for (int r = 0; r < nk; ++r) acc = fma(-Hl[i * ld + nx + r], src[r * ld + tx], acc);
      Pl[i * ldp + tx] = acc;
    }
    __syncthreads();
    const double* Kf = src;                                                // K_j [mb x nx], leading dimension ld: without a constraint-to-go K is final
    if (c > 0) {                                                           // ---- the projection: Pz in C0, (.) Pz in C1, K Pz into the free solve buffer, Pz (.) Pz
      if (tx < nx) for (int i = ty; i < nx; i += rs) {
        double acc = (i == tx) ? 1.0 : 0.0;
        for (int q = 0; q < c; ++q) acc = fma(-HnC[q * ldp + i], HnC[q * ldp + tx], acc);
        C0[i * ldc + tx] = acc;
      }
      __syncthreads();
      if (tx < nx) {
        for (int i = ty; i < nx; i += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(Pl[i * ldp + s], C0[s * ldc + tx], acc);
          C1[i * ldc + tx] = acc;
        }
        for (int r = ty; r < mb; r += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(src[r * ld + s], C0[s * ldc + tx], acc);
          dst[r * ld + tx] = acc;
        }
      }
      __syncthreads();
      if (tx < nx) for (int i = ty; i < nx; i += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(C0[i * ldc + s], C1[s * ldc + tx], acc);
        Pl[i * ldp + tx] = acc;
      }
      __syncthreads();
      Kf = dst;
    }
    // ---- feasibility of the stage: the stack once more into C1, [Cx - Cu K_j] in place, times Pz_j (C0; the identity when c = 0)
    if (m > 0) {
      if (tx < n) {
        for (int i = ty; i < me; i += rs) C1[i * ldc + tx] = Jk[i * n + tx];
        for (int i = ty; i < md; i += rs) if (clsl[i] == 1) C1[(me + posl[i]) * ldc + tx] = Dk[i * n + tx];
        for (int i = ty; i < cn; i += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(HnN[i * ldp + s], El[s * ld + tx], acc);
          C1[(rk + i) * ldc + tx] = acc;
        }
      }
      __syncthreads();
      if (tx < nx) for (int i = ty; i < m; i += rs) {
        double acc = C1[i * ldc + tx];
        for (int r = 0; r < mb; ++r) acc = fma(-C1[i * ldc + nx + r], Kf[r * ld + tx], acc);
        C1[i * ldc + tx] = acc;
      }
      __syncthreads();
      if (tx < nx) for (int i = ty; i < m; i += rs) {
        double acc = C1[i * ldc + tx];
        if (c > 0) {
          acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(C1[i * ldc + s], C0[s * ldc + tx], acc);
        }
        feas = fmax(feas, fabs(acc));
      }
    }
    // ---- K_j, c_j out; Pi_j = sym(.)
    double bad = 0.0;
    if (tx < nx) {
      if (Kall) for (int r = ty; r < mb; r += rs) Kall[((size_t)j * mb + r) * nx + tx] = Kf[r * ld + tx];
      if (j == 0) {
        for (int r = ty; r < mb; r += rs) K0[r * nx + tx] = Kf[r * ld + tx];
        for (int i = ty; i < nx; i += rs) Hn0[i * nx + tx] = i < c ? HnC[i * ldp + tx] : 0.0;
      }
      for (int i = ty; i <= tx; i += rs) {                                 // the pair (i, tx), i <= tx, belongs to one thread
        const double val = 0.5 * (Pl[i * ldp + tx] + Pl[tx * ldp + i]);
        if (!(fabs(val) < INFINITY)) bad = 1.0;
        Pl[i * ldp + tx] = val; Pl[tx * ldp + i] = val;
        if (j == 0) { Pi0[i * nx + tx] = val; Pi0[tx * nx + i] = val; }
      }
    }
    if (tid == 0 && cntall) cntall[j] = c;
    bad = lqr_wave_max(bad);
    if (lane == 0) red[wv] = bad;
    __syncthreads();
    bad = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    { double* t_ = HnN; HnN = HnC; HnC = t_; }
    cn = c;
    if (bad > 0.0) { status = LQR_NONFINITE; break; }
    csum += c; cmax = max(cmax, c);
    done = N - j;
  }
  feas = lqr_wave_max(feas);
  strict = -lqr_wave_max(-strict);
  if (lane == 0) { red[8 + wv] = feas; red[12 + wv] = strict; }            // (slots of their own: a pass that broke off may still have readers of red[0 .. 3])
  __syncthreads();
  double* o = a.info + bi * LQR_CTG_INFO;
  if (tid == 0) {
    o[0] = status; o[1] = N; o[2] = done; o[3] = pmin; o[4] = pmax; o[5] = (status == LQR_OK) ? posdef : 0.0; o[6] = (status == LQR_OK) ? posdef : 0.0;
    o[7] = (status == LQR_OK) ? fmax(fmax(red[8], red[9]), fmax(red[10], red[11])) : 0.0;
    o[8] = csum; o[9] = cmax; o[10] = accmin; o[11] = rejmax;
    a.cnt0[bi] = (status == LQR_OK) ? cn : cfail;
    if (a.strict) {
      const double sm = fmin(fmin(red[12], red[13]), fmin(red[14], red[15]));
      a.strict[bi] = (status == LQR_OK) ? (sm < INFINITY ? sm : 1.0) : qnan;       // (no pair at all: nothing is ambiguous)
    }
  }
  if (status != LQR_OK) {                                                  // nothing to return for this instance; the stages it did not finish
    for (int e = tid; e < mb * nx; e += LQR_NT) K0[e] = qnan;
    for (int e = tid; e < nx * nx; e += LQR_NT) { Pi0[e] = qnan; Hn0[e] = 0.0; }
    const int left = N - done;
    if (Kall) for (size_t e = tid; e < (size_t)left * mb * nx; e += LQR_NT) Kall[e] = qnan;
    if (cntall) for (int e = tid; e < left; e += LQR_NT) cntall[e] = -1;
    if (clso) for (int e = tid; e < left * nd; e += LQR_NT) clso[e] = -1;
    if (a.dX) {
      double* dX = a.dX + bi * (size_t)(N + 1) * nx * nx; double* dU = a.dU + bi * (size_t)N * mb * nx;
      for (size_t e = tid; e < (size_t)(N + 1) * nx * nx; e += LQR_NT) dX[e] = qnan;
      for (size_t e = tid; e < (size_t)N * mb * nx; e += LQR_NT) dU[e] = qnan;
    }
    return;
  }
  if (!a.dX) return;
  // ---- the open-loop sensitivities: Phi ping-pong between the Pi and W buffers, K_j in the Hb buffer, dU_j in C0; Hn_0 stands in HnN
  double* dX = a.dX + bi * (size_t)(N + 1) * nx * nx; double* dU = a.dU + bi * (size_t)N * mb * nx;
  double* F = Pl; double* Fn = Wl; double* Kl = Hl;
  __syncthreads();
  if (tx < nx) for (int r = ty; r < nx; r += rs) {
    double acc = (r == tx) ? 1.0 : 0.0;
    for (int q = 0; q < cn; ++q) acc = fma(-HnN[q * ldp + r], HnN[q * ldp + tx], acc);
    F[r * ldp + tx] = acc;
    dX[r * nx + tx] = acc;
  }
  for (int j = 0; j < N; ++j) {
    const int k = (k0 + j % p) % p;
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Kj = Kall + (size_t)j * mb * nx;
    if (tx < n) for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
    if (tx < nx) for (int r = ty; r < mb; r += rs) Kl[r * ldp + tx] = Kj[r * nx + tx];
    __syncthreads();
    if (tx < nx) for (int r = ty; r < mb; r += rs) {
      double acc = 0.0;
      for (int s = 0; s < nx; ++s) acc = fma(-Kl[r * ldp + s], F[s * ldp + tx], acc);
      C0[r * ldc + tx] = acc;
      dU[((size_t)j * mb + r) * nx + tx] = acc;
    }
    __syncthreads();
    if (tx < nx) for (int i = ty; i < nx; i += rs) {
      double acc = 0.0;
      for (int s = 0; s < nx; ++s) acc = fma(El[i * ld + s], F[s * ldp + tx], acc);
      for (int r = 0; r < mb; ++r) acc = fma(El[i * ld + nx + r], C0[r * ldc + tx], acc);
      Fn[i * ldp + tx] = acc;
      dX[((size_t)(j + 1) * nx + i) * nx + tx] = acc;
    }
    __syncthreads();
    double* t_ = F; F = Fn; Fn = t_;
  }
}

}  // namespace tmpc
