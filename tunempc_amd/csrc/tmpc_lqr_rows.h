// Periodic LQR gains with the rows of G_k / C_k held as equalities: the recursion of tmpc_lqr.h for the models with rows (reference: convexifier.py:44-45 read
// with :249-266 -- Hc_k = H_k + calH_k(P) + J_k' diag(phi_k) J_k, and the last term vanishes on J_k w = 0, so the LQ problems on H and on Hc that hold
// J_k [x_k; u_k] = 0 at every stage share their feedback law; the unconstrained ones do not once a multiplier is non-zero).
// Stage k carries r_k = ng + ncnt_k rows J_k = [Jx | Ju] (first nx | last mb columns; the J / ncnt layout of tmpc_convexify_step2_batch_host):
//     E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,
//     [ S   Ju' ] [ K   ]   [ M  ]
//     [ Ju  0   ] [ Lam ] = [ Jx ]          u = -K_k x,   Pi_k = sym( Hb_xx - [M; Jx]' [K; Lam] ),        Jx - Ju K_k = 0.
// Served: stages whose Ju has full row rank (r_k <= mb: every x is feasible and the cost-to-go is a quadratic form on all of R^nx).  r_k > mb at any stage
// ends the problem with status 4 before the first sweep; a rank-deficient Ju or a singular reduced Hessian with status 2 through the relative pivot test.
// Rows that constrain the state alone (Ju = 0) need a constraint-to-go recursion: not served (they end with status 2).
//
// Residency and arithmetic are those of k_periodic_lqr: one 256-thread workgroup per problem, every sweep, the stop test and the monodromy in one launch, fp64 on
// the vector ALU, Pi_k handed on in LDS.  The Hb buffer is bordered, [[Hb, J'], [J, 0]] with leading dimension (n + nr) | 1, so that its rows nx .. n + r_k - 1
// ARE the block [M; Jx | KKT] of (mb + r_k) x (nx + mb + r_k): J_k is one more operand load, the elimination runs in place (ping-pong with the W buffer, one
// barrier per pivot) and [M; Jx]' stays readable in the rows above it for the Pi update.  A stage is 6 + mb + r_k barrier-separated steps; r_k follows ncnt
// stage by stage, nothing is padded with fake rows, and with r_k = 0 everywhere the arithmetic is that of k_periodic_lqr, operation for operation.
//
// Pivot rule: in the first mb columns the diagonal entry when it is positive and at least LQR_PIV_THRESH of the column maximum, in the r_k multiplier columns
// when it is NEGATIVE and at least that large in magnitude, else the column maximum.  An elimination that took mb positive and then r_k negative diagonal
// pivots proves S positive definite and Ju of full row rank (the Schur complement -Ju S^-1 Ju' is negative definite): a convex stage problem -- info[5] for
// the last sweep, info[6] for the whole path.  On the Hc side every stage must show it; on the H side S is indefinite in general and the column maximum is
// the normal case.
//
// LDS (lqr_rows_lds, host and device): E [nx x ld], Pi [nx x (nx | 1)], W [max(nx, mb + nr) x ld], bordered Hb [(n + nr) x ld], ld = (n + nr) | 1: 30 KB at the
// bench stage shape with 5 rows (26 KB without rows: the layout of lqr_lds).  What fits 160 KB is served, the rest refused with TMPC_E_UNSUPPORTED before the
// device is touched: every n <= 32 with any row capacity nr <= 66 (so any r <= mb); for 32 < n <= 64 every nr <= 15 whatever the split of n, and more where the
// split leaves room (nx = mb = nr = 32: 157 KB fits; nx = 40, mb = nr = 24 fits; nx = 1, mb = 63 stops at nr = 28).
#pragma once
#include "tmpc_lqr.h"

namespace tmpc {

enum { LQR_ROWS_EXCEED = 4 };
constexpr int LQR_LDS_BYTES = 160 * 1024;

struct LqrRowsLds { int ld, ldp, oE, oP, oW, oH, oR, total; };      // offsets in doubles; nr = 0 gives the layout of lqr_lds
__host__ __device__ inline LqrRowsLds lqr_rows_lds(int nx, int mb, int nr) {
  LqrRowsLds l;
  const int n = nx + mb, nk = mb + nr, mr = nx > nk ? nx : nk;
  l.ld = (n + nr) | 1; l.ldp = nx | 1;
  l.oE = 0;                            // E_k [nx x n]
  l.oP = l.oE + nx * l.ld;             // Pi_{k+1} [nx x nx], then Hb_xx - [M; Jx]' [K; Lam], then Pi_k
  l.oW = l.oP + nx * l.ldp;            // W = Pi E [nx x n]; second buffer of the elimination [(mb + r) x (n + r)]
  l.oH = l.oW + mr * l.ld;             // [[Hb, J'], [J, 0]]  [(n + r) x (n + r)]
  l.oR = l.oH + (n + nr) * l.ld;       // block reductions
  l.total = l.oR + 16;
  return l;
}

__device__ __forceinline__ int lqr_wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// grid: nb workgroups.  cw: power of two >= n (<= 64), the column width of the thread layout; lcw = log2 cw.  J [nb][p][nr][n], ncnt [nb][p] or null (ng rows everywhere).
__global__ void __launch_bounds__(LQR_NT) k_periodic_lqr_rows(int p, int nx, int mb, int nr, int ng, int lcw, const double* __restrict__ Ag,
                                                              const double* __restrict__ Bg, const double* __restrict__ Hg, const double* __restrict__ Jg,
                                                              const int* __restrict__ ncntg, const double* __restrict__ Pi0, double tol, int max_sweeps,
                                                              double* __restrict__ Kg, double* Pig, double* __restrict__ Phig, double* __restrict__ Lamg,
                                                              double* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const LqrRowsLds L = lqr_rows_lds(nx, mb, nr);
  const int ld = L.ld, ldp = L.ldp;
  double* El = lds + L.oE; double* Pl = lds + L.oP; double* Wl = lds + L.oW; double* Hl = lds + L.oH; double* red = lds + L.oR;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const size_t b = blockIdx.x;
  const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* H = Hg + b * p * n * n;
  const double* J = Jg + b * p * nr * n; const int* ncnt = ncntg ? ncntg + b * p : nullptr;
  double* K = Kg + b * p * mb * nx; double* Pi = Pig + b * p * nx * nx; double* Lam = Lamg ? Lamg + b * p * nr * nx : nullptr;
  const int pnn = p * nx * nx;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- the row counts of every stage, before anything is solved: beyond the inputs (or the capacity of J) -> status 4
  if (tid == 0) red[8] = 0.0;
  __syncthreads();
  {
    bool bad = false;
    for (int k = tid; k < p; k += LQR_NT) {
      const int c = ncnt ? ncnt[k] : 0;
      bad = bad || c < 0 || ng + c > nr || ng + c > mb;
    }
    if (bad) red[8] = 1.0;
  }
  for (int e = tid; e < pnn; e += LQR_NT) Pi[e] = Pi0 ? Pi0[b * pnn + e] : 0.0;
  __syncthreads();
  if (red[8] != 0.0) {                                                        // K, Lam zero, Pi = Pi0, Phi NaN, no sweep
    for (int e = tid; e < p * mb * nx; e += LQR_NT) K[e] = 0.0;
    if (Lam) for (int e = tid; e < p * nr * nx; e += LQR_NT) Lam[e] = 0.0;
    if (Phig) for (int e = tid; e < nx * nx; e += LQR_NT) Phig[b * nx * nx + e] = qnan;
    if (tid == 0) {
      double* o = info + b * 8;
      o[0] = LQR_ROWS_EXCEED; o[1] = 0.0; o[2] = 0.0; o[3] = INFINITY; o[4] = 0.0; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0;
    }
    return;
  }

  int status = LQR_MAXSWEEPS, sweeps = 0;
  double rel = 0.0, pmin = INFINITY, pmax = 0.0, posdef = 1.0, posdef_path = 1.0;
  for (int sw = 0; sw < max_sweeps && status == LQR_MAXSWEEPS; ++sw) {
    rel = 0.0; pmin = INFINITY; pmax = 0.0; posdef = 1.0;
    for (int k = p - 1; k >= 0; --k) {
      const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Hk = H + (size_t)k * n * n;
      const double* Jk = J + (size_t)k * nr * n;
      const int rk = ng + (ncnt ? ncnt[k] : 0), nk = mb + rk, wid = n + rk;
      // ---- operands of the stage
      if (k == p - 1) {                                                     // (every other stage finds Pi_{k+1} where the last one left it)
        const double* Pn = Pi + (size_t)((k + 1) % p) * nx * nx;
        if (tx < nx) for (int r = ty; r < nx; r += rs) Pl[r * ldp + tx] = Pn[r * nx + tx];
      }
      if (tx < n) {
        for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
        for (int r = ty; r < n; r += rs) Hl[r * ld + tx] = Hk[r * n + tx];
        for (int j = ty; j < rk; j += rs) {                                   // the border: J_k below Hb, J_k' beside it
          const double v = Jk[j * n + tx];
          Hl[(n + j) * ld + tx] = v; Hl[tx * ld + n + j] = v;
        }
      }
      if (tx < rk) for (int j = ty; j < rk; j += rs) Hl[(n + j) * ld + n + tx] = 0.0;
      __syncthreads();
      // ---- W = Pi_{k+1} E
      if (tx < n) for (int r = ty; r < nx; r += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(Pl[r * ldp + s], El[s * ld + tx], acc);
        Wl[r * ld + tx] = acc;
      }
      __syncthreads();
      // ---- Hb = H_k + E' W
      if (tx < n) for (int i = ty; i < n; i += rs) {
        double acc = Hl[i * ld + tx];
        for (int r = 0; r < nx; ++r) acc = fma(El[r * ld + i], Wl[r * ld + tx], acc);
        Hl[i * ld + tx] = acc;
      }
      __syncthreads();
      // ---- [M; Jx | S Ju'; Ju 0] -> [K; Lam | I]: one pivot per barrier, src -> dst
      double* src = Hl + nx * ld; double* dst = Wl;
      double spmax = 0.0;
      for (int c = 0; c < nk; ++c) {
        const int pc = nx + c, rem = nk - c;
        double v = -1.0; int vi = 0;                                         // every wave finds the pivot for itself: no barrier for the search
        for (int q = lane; q < rem; q += 64) {
          double a = fabs(src[(c + q) * ld + pc]);
          if (a != a) a = INFINITY;
          if (a > v) { v = a; vi = q; }
        }
        const double vmax = lqr_wave_max(v);
        int pr;
        if (rem <= 64) pr = c + __ffsll((long long)__ballot(v == vmax)) - 1;
        else pr = c + lqr_wave_min(v == vmax ? vi : 0x7fffffff);             // (more than 64 rows: the first row that holds the maximum, as above)
        const double diag = src[c * ld + pc];
        const bool keep = c < mb ? (diag > 0.0 && diag >= LQR_PIV_THRESH * vmax) : (diag < 0.0 && -diag >= LQR_PIV_THRESH * vmax);
        if (keep) pr = c; else { posdef = 0.0; posdef_path = 0.0; }
        const double pv = src[pr * ld + pc], apv = fabs(pv);
        if (!(apv < INFINITY)) { status = LQR_NONFINITE; break; }
        if (!(apv > LQR_SING_REL * spmax)) { status = LQR_SINGULAR; pmin = fmin(pmin, apv); break; }
        spmax = fmax(spmax, apv); pmin = fmin(pmin, apv); pmax = fmax(pmax, apv);
        const double inv = 1.0 / pv;
        for (int col = tx; col < wid; col += cw) {
          if (col >= nx && col <= pc) continue;                              // (the columns of the KKT matrix already reduced are never read again)
          const double pj = src[pr * ld + col] * inv;
          for (int r = ty; r < nk; r += rs) {
            const int q = (r == pr) ? c : r;                                 // row pr receives what stood in row c
            dst[r * ld + col] = (r == c) ? pj : fma(-src[q * ld + pc], pj, src[q * ld + col]);
          }
        }
        __syncthreads();
        double* t_ = src; src = dst; dst = t_;
      }
      if (status != LQR_MAXSWEEPS) break;                                    // (uniform: every thread read the same pivots)
      // ---- K_k, Lam_k out; Hb_xx - [M; Jx]' [K_k; Lam_k]
      if (tx < nx) {
        double* Kk = K + (size_t)k * mb * nx;
        for (int r = ty; r < mb; r += rs) Kk[r * nx + tx] = src[r * ld + tx];
        if (Lam) {
          double* Lk = Lam + (size_t)k * nr * nx;
          for (int j = ty; j < nr; j += rs) Lk[j * nx + tx] = j < rk ? src[(mb + j) * ld + tx] : 0.0;
        }
        for (int i = ty; i < nx; i += rs) {
          double acc = Hl[i * ld + tx];
          for (int r = 0; r < nk; ++r) acc = fma(-Hl[i * ld + nx + r], src[r * ld + tx], acc);
          Pl[i * ldp + tx] = acc;
        }
      }
      __syncthreads();
      // ---- Pi_k = sym(.), its change against the last sweep
      double dmax = 0.0, vabs = 0.0;
      if (tx < nx) {
        double* Pk = Pi + (size_t)k * nx * nx;
        for (int i = ty; i <= tx; i += rs) {                                 // the pair (i, tx), i <= tx, belongs to one thread
          const double val = 0.5 * (Pl[i * ldp + tx] + Pl[tx * ldp + i]);
          double d = fmax(fabs(val - Pk[i * nx + tx]), fabs(val - Pk[tx * nx + i]));
          if (!(fabs(val) < INFINITY) || d != d) d = INFINITY;
          dmax = fmax(dmax, d); vabs = fmax(vabs, fabs(val));
          Pl[i * ldp + tx] = val; Pl[tx * ldp + i] = val;
          Pk[i * nx + tx] = val; Pk[tx * nx + i] = val;
        }
      }
      dmax = lqr_wave_max(dmax); vabs = lqr_wave_max(vabs);
      if (lane == 0) { red[wv] = dmax; red[4 + wv] = vabs; }
      __syncthreads();
      dmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
      vabs = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
      if (!(dmax < INFINITY)) { status = LQR_NONFINITE; rel = INFINITY; break; }
      rel = fmax(rel, dmax / fmax(1.0, vabs));
    }
    if (status != LQR_MAXSWEEPS) break;
    sweeps = sw + 1;
    if (rel <= tol) status = LQR_OK;
  }
  if (status >= LQR_SINGULAR) sweeps += 1;                                   // the sweep that failed counts
  double* o = info + b * 8;
  if (tid == 0) {
    o[0] = status; o[1] = sweeps; o[2] = rel; o[3] = pmin; o[4] = pmax; o[5] = (status <= LQR_MAXSWEEPS) ? posdef : 0.0; o[6] = (status <= LQR_MAXSWEEPS) ? posdef_path : 0.0; o[7] = 0.0;
  }
  if (status >= LQR_SINGULAR) {                                              // no closed loop to speak of
    if (Phig) for (int e = tid; e < nx * nx; e += LQR_NT) Phig[b * nx * nx + e] = qnan;
    return;
  }
  // ---- monodromy Phi = (A_{p-1} - B_{p-1} K_{p-1}) ... (A_0 - B_0 K_0) and the feasibility of the gains, max |Jx - Ju K_k|: Acl and K_k in the Hb buffer,
  //      Phi ping-pong between the Pi and W buffers
  __syncthreads();
  double* F = Pl; double* Fn = Wl; double* Acl = Hl; double* Kl = Hl + nx * ldp;
  double feas = 0.0;
  if (tx < nx) for (int r = ty; r < nx; r += rs) F[r * ldp + tx] = (r == tx) ? 1.0 : 0.0;
  for (int k = 0; k < p; ++k) {
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Kk = K + (size_t)k * mb * nx;
    const double* Jk = J + (size_t)k * nr * n;
    const int rk = ng + (ncnt ? ncnt[k] : 0);
    if (tx < n) for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
    if (tx < nx) for (int r = ty; r < mb; r += rs) Kl[r * nx + tx] = Kk[r * nx + tx];
    __syncthreads();
    if (tx < nx) {
      for (int j = ty; j < rk; j += rs) {
        double acc = Jk[j * n + tx];
        for (int r = 0; r < mb; ++r) acc = fma(-Jk[j * n + nx + r], Kl[r * nx + tx], acc);
        feas = fmax(feas, fabs(acc));
      }
      if (Phig) for (int i = ty; i < nx; i += rs) {
        double acc = El[i * ld + tx];
        for (int r = 0; r < mb; ++r) acc = fma(-El[i * ld + nx + r], Kl[r * nx + tx], acc);
        Acl[i * ldp + tx] = acc;
      }
    }
    __syncthreads();
    if (Phig && tx < nx) for (int i = ty; i < nx; i += rs) {
      double acc = 0.0;
      for (int s = 0; s < nx; ++s) acc = fma(Acl[i * ldp + s], F[s * ldp + tx], acc);
      Fn[i * ldp + tx] = acc;
    }
    __syncthreads();
    double* t_ = F; F = Fn; Fn = t_;
  }
  if (Phig && tx < nx) for (int r = ty; r < nx; r += rs) Phig[b * nx * nx + r * nx + tx] = F[r * ldp + tx];
  feas = lqr_wave_max(feas);
  if (lane == 0) red[wv] = feas;
  __syncthreads();
  if (tid == 0) o[7] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

}  // namespace tmpc
