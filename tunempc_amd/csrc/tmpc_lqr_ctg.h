// Periodic LQR gains with the rows J_k = [G_k; C_k] held as equalities when the rows need not fit the inputs: more rows than inputs, rows on the state
// alone, dependent rows.  The recursion of tmpc_lqr_rows.h carries one more quantity per stage, a constraint-to-go Hn_k (c_k orthonormal rows of length nx,
// Hn_k x_k = 0, empty at the start).  Stage k, indices mod p:
//   1. stack    Cf = [J_k (first r_k rows); Hn_{k+1} [A_k B_k]] = [Cx | Cu],  m = r_k + c_{k+1} rows;
//   2. split    elimination on the Cu columns with FULL pivoting (largest remaining |entry| of the Cu block), until that maximum is <= rank_tol * max(1, max|Cf|):
//               the rho <= mb pivot rows, in echelon form, are a full-row-rank [Jx~ | Ju~]; the other rows have a zero u part;
//   3. compress their x parts by Gram-Schmidt with row pivoting (largest remaining 2-norm, same threshold) to Hn_k, c_k orthonormal rows;
//               c_k = nx ends the problem with status 5: no feasible subspace;
//   4. solve    [[S, Ju~'], [Ju~, 0]] [K; Lam] = [M; Jx~] by the bordered in-place Gauss-Jordan of k_periodic_lqr_rows (same pivot rule, rho = mb allowed);
//               each row of [Jx~ | Ju~] enters the border scaled so that its pivot equals the largest diagonal entry of S (a homogeneous equality may be scaled
//               freely: K and [M; Jx~]' [K; Lam] do not change).  Without it the multiplier pivots, -Ju~ S^-1 Ju~', sit at 1 / |S| next to pivots of S at |S|, and
//               at |Pi| = 1e8 the relative singularity test of the elimination (LQR_SING_REL) ends a well-posed stage with status 2;
//   5. project  Pz = I - Hn_k' Hn_k,  K_k = K Pz,  Pi_k = sym(Pz (Hb_xx - [M; Jx~]' [K; Lam]) Pz): off the feasible subspace both are arbitrary, the
//               projection makes them unique.  (The multipliers are not unique and are not returned.)
// Sweeps stop when max|dPi_k| / max(1, max|Pi_k|) <= tol AND no c_k changed during the sweep (counts only grow from the empty start, by at most p nx in all).
// Monodromy pass: Phi = (A-BK)_{p-1} ... (A-BK)_0 Pz_0 and feas = max_k max(|(Jx - Ju K_k) Pz_k|, |Hn_{k+1} (A_k - B_k K_k) Pz_k|).
//
// Residency is that of k_periodic_lqr_rows: one 256-thread workgroup per problem, the whole iteration in one launch, every operand of a stage in LDS, fp64 on
// the vector ALU, every wave finds each pivot for itself, one barrier per pivot (split, compression and solve all ping-pong between two buffers: a step reads
// one and writes the other, so no wave can see a row another wave has already updated).  A pivot row of the split is final when it is chosen and goes straight
// into the border of the Hb buffer (below Hb and, transposed, beside it); only the rows below it are carried on.  Hn_k stays in LDS as the Hn_{k+1} of the next
// stage, as Pi does; all Hn_k and c_k also live in the global outputs, read back at the wrap-around stage and by the monodromy pass.
//
// The border holds at most nbd = min(mb, nr + nx) rows, so ld = (n + nbd) | 1.  LDS (lqr_ctg_lds): E [nx x ld], Pi [nx x (nx|1)], W [max(nx, mb + nbd) x ld],
// bordered Hb [(n + nbd) x ld], two stack buffers [max(nr + nx, mb) x (n|1)] (later Pz and Pi Pz), Hn_{k+1} and Hn_k [nx x (nx|1)] each: 61 KB at the bench
// stage shape with room for 10 rows.  What exceeds 160 KB is refused with TMPC_E_UNSUPPORTED before the device is touched.
// Orthogonality of Hn_k: one Gram-Schmidt pass, so Hn_k Hn_k' - I is of the order of eps / (smallest accepted pivot, info[10]).
#pragma once
#include "tmpc_lqr_rows.h"

namespace tmpc {

enum { LQR_NO_FEASIBLE = 5 };
constexpr int LQR_CTG_INFO = 12;             // doubles of info per problem (TMPC_LQR_CTG_INFO)

struct LqrCtgLds { int ld, ldp, ldc, nbd, ms, oE, oP, oW, oH, oC0, oC1, oN0, oN1, oR, total; };      // offsets in doubles
__host__ __device__ inline LqrCtgLds lqr_ctg_lds(int nx, int mb, int nr) {
  LqrCtgLds l;
  const int n = nx + mb;
  l.nbd = mb < nr + nx ? mb : nr + nx;
  l.ms = nr + nx > mb ? nr + nx : mb;
  const int nk = mb + l.nbd, mr = nx > nk ? nx : nk;
  l.ld = (n + l.nbd) | 1; l.ldp = nx | 1; l.ldc = n | 1;
  l.oE = 0;                               // E_k [nx x n]
  l.oP = l.oE + nx * l.ld;                // Pi_{k+1}, then Hb_xx - [M; Jx~]' [K; Lam], then Pi_k
  l.oW = l.oP + nx * l.ldp;               // W = Pi E; second buffer of the solve [(mb + rho) x (n + rho)]
  l.oH = l.oW + mr * l.ld;                // [[Hb, J~'], [J~, 0]]
  l.oC0 = l.oH + (n + l.nbd) * l.ld;      // the stack [m x n], ping
  l.oC1 = l.oC0 + l.ms * l.ldc;           // pong
  l.oN0 = l.oC1 + l.ms * l.ldc;           // Hn_{k+1} [c x nx]
  l.oN1 = l.oN0 + nx * l.ldp;             // Hn_k
  l.oR = l.oN1 + nx * l.ldp;              // block reductions
  l.total = l.oR + 16;
  return l;
}

// grid: nb workgroups.  cw, lcw as in k_periodic_lqr_rows.  J [nb][p][nr][n], ncnt [nb][p] or null (ng rows everywhere; counts are clamped to 0 .. nr).
// Outputs: K [nb][p][mb][nx], Pi [nb][p][nx][nx], Phi [nb][nx][nx] or null, Hn [nb][p][nx][nx] (rows beyond c_k zero), cnt [nb][p], info [nb][12].
__global__ void __launch_bounds__(LQR_NT) k_periodic_lqr_ctg(int p, int nx, int mb, int nr, int ng, int lcw, const double* __restrict__ Ag,
                                                             const double* __restrict__ Bg, const double* __restrict__ Hg, const double* __restrict__ Jg,
                                                             const int* __restrict__ ncntg, const double* __restrict__ Pi0, double tol, double rank_tol,
                                                             int max_sweeps, double* __restrict__ Kg, double* Pig, double* __restrict__ Phig, double* Hng,
                                                             int* cntg, double* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const LqrCtgLds L = lqr_ctg_lds(nx, mb, nr);
  const int ld = L.ld, ldp = L.ldp, ldc = L.ldc, nbd = L.nbd;
  double* El = lds + L.oE; double* Pl = lds + L.oP; double* Wl = lds + L.oW; double* Hl = lds + L.oH; double* red = lds + L.oR;
  double* C0 = lds + L.oC0; double* C1 = lds + L.oC1; double* HnN = lds + L.oN0; double* HnC = lds + L.oN1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const size_t b = blockIdx.x;
  const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* H = Hg + b * p * n * n;
  const double* J = Jg + b * p * nr * n; const int* ncnt = ncntg ? ncntg + b * p : nullptr;
  double* K = Kg + b * p * mb * nx; double* Pi = Pig + b * p * nx * nx; double* Hn = Hng + b * p * nx * nx; int* cnt = cntg + b * p;
  const int pnn = p * nx * nx;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  for (int e = tid; e < pnn; e += LQR_NT) { Pi[e] = Pi0 ? Pi0[b * pnn + e] : 0.0; Hn[e] = 0.0; }
  for (int k = tid; k < p; k += LQR_NT) cnt[k] = 0;
  __syncthreads();

  int status = LQR_MAXSWEEPS, sweeps = 0, cn = 0, csum = 0, cmax = 0;
  double rel = 0.0, pmin = INFINITY, pmax = 0.0, posdef = 1.0, posdef_path = 1.0, accmin = INFINITY, rejmax = 0.0;
  for (int sw = 0; sw < max_sweeps && status == LQR_MAXSWEEPS; ++sw) {
    rel = 0.0; pmin = INFINITY; pmax = 0.0; posdef = 1.0; csum = 0; cmax = 0;
    bool changed = false;
    for (int k = p - 1; k >= 0; --k) {
      const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Hk = H + (size_t)k * n * n;
      const double* Jk = J + (size_t)k * nr * n;
      const int rk = max(0, min(nr, ng + (ncnt ? ncnt[k] : 0)));
      const int cold = cnt[k];
      // ---- operands of the stage
      if (k == p - 1) {                                                     // (every other stage finds Pi_{k+1}, Hn_{k+1} where the last one left them)
        const int kn = (k + 1) % p;
        const double* Pn = Pi + (size_t)kn * nx * nx; const double* Nn = Hn + (size_t)kn * nx * nx;
        cn = cnt[kn];
        if (tx < nx) {
          for (int r = ty; r < nx; r += rs) Pl[r * ldp + tx] = Pn[r * nx + tx];
          for (int r = ty; r < cn; r += rs) HnN[r * ldp + tx] = Nn[r * nx + tx];
        }
      }
      if (tx < n) {
        for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
        for (int r = ty; r < n; r += rs) Hl[r * ld + tx] = Hk[r * n + tx];
        for (int j = ty; j < rk; j += rs) C0[j * ldc + tx] = Jk[j * n + tx];
      }
      if (tx < nbd) for (int j = ty; j < nbd; j += rs) Hl[(n + j) * ld + n + tx] = 0.0;
      __syncthreads();
      // ---- W = Pi_{k+1} E; the constraint-to-go seen from stage k, Hn_{k+1} E, below the rows of J_k
      if (tx < n) {
        for (int r = ty; r < nx; r += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(Pl[r * ldp + s], El[s * ld + tx], acc);
          Wl[r * ld + tx] = acc;
        }
        for (int j = ty; j < cn; j += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(HnN[j * ldp + s], El[s * ld + tx], acc);
          C0[(rk + j) * ldc + tx] = acc;
        }
      }
      __syncthreads();
      // ---- Hb = H_k + E' W
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
          double a = fabs(cs[i * ldc + q - i * n]);
          if (a != a) a = INFINITY;
          v = fmax(v, a);
        }
        const double scale = fmax(1.0, lqr_wave_max(v));
        if (!(scale < INFINITY)) { status = LQR_NONFINITE; break; }
        const double thr = rank_tol * scale;
        double sfac = (lane < mb) ? fabs(Hl[(nx + lane) * ld + nx + lane]) : 0.0;      // the scale of S: its largest diagonal entry
        sfac = lqr_wave_max(sfac);
        if (!(sfac > 0.0 && sfac < INFINITY)) sfac = 1.0;
        for (;;) {                                                           // the split: full pivoting on the Cu block of the rows rho .. m-1
          const int rem = m - rho;
          if (rem == 0) break;
          double vb = -1.0; int vi = 0;
          for (int q = lane; q < rem * mb; q += 64) {
            const int i = q / mb;
            const double a = fabs(cs[(rho + i) * ldc + nx + q - i * mb]);
            if (a > vb) { vb = a; vi = q; }
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
          if (c + 1 == nx) { status = LQR_NO_FEASIBLE; c = nx; break; }       // x_k = 0 is all that is left
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
      changed = changed || c != cold;
      csum += c; cmax = max(cmax, c);
      if (status != LQR_MAXSWEEPS) break;
      const int nk = mb + rho, wid = n + rho;
      // ---- [M; Jx~ | S Ju~'; Ju~ 0] -> [K; Lam | I]: one pivot per barrier, src -> dst
      double* src = Hl + nx * ld; double* dst = Wl;
      double spmax = 0.0;
      for (int cc = 0; cc < nk; ++cc) {
        const int pc = nx + cc, rem = nk - cc;
        double v = -1.0; int vi = 0;
        for (int q = lane; q < rem; q += 64) {
          double a = fabs(src[(cc + q) * ld + pc]);
          if (a != a) a = INFINITY;
          if (a > v) { v = a; vi = q; }
        }
        const double vmax = lqr_wave_max(v);
        int pr;
        if (rem <= 64) pr = cc + __ffsll((long long)__ballot(v == vmax)) - 1;
        else pr = cc + lqr_wave_min(v == vmax ? vi : 0x7fffffff);
        const double diag = src[cc * ld + pc];
        const bool keep = cc < mb ? (diag > 0.0 && diag >= LQR_PIV_THRESH * vmax) : (diag < 0.0 && -diag >= LQR_PIV_THRESH * vmax);
        if (keep) pr = cc; else { posdef = 0.0; posdef_path = 0.0; }
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
      if (status != LQR_MAXSWEEPS) break;
      // ---- Hb_xx - [M; Jx~]' [K; Lam]; without a constraint-to-go K is final
      double* Kk = K + (size_t)k * mb * nx;
      if (tx < nx) {
        if (c == 0) for (int r = ty; r < mb; r += rs) Kk[r * nx + tx] = src[r * ld + tx];
        for (int i = ty; i < nx; i += rs) {
          double acc = Hl[i * ld + tx];
          for (int r = 0; r < nk; ++r) acc = fma(-Hl[i * ld + nx + r], src[r * ld + tx], acc);
          Pl[i * ldp + tx] = acc;
        }
      }
      __syncthreads();
      if (c > 0) {                                                           // ---- the projection: Pz in C0, (.) Pz in C1, K Pz out, Pz (.) Pz
        if (tx < nx) for (int i = ty; i < nx; i += rs) {
          double acc = (i == tx) ? 1.0 : 0.0;
          for (int j = 0; j < c; ++j) acc = fma(-HnC[j * ldp + i], HnC[j * ldp + tx], acc);
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
            Kk[r * nx + tx] = acc;
          }
        }
        __syncthreads();
        if (tx < nx) for (int i = ty; i < nx; i += rs) {
          double acc = 0.0;
          for (int s = 0; s < nx; ++s) acc = fma(C0[i * ldc + s], C1[s * ldc + tx], acc);
          Pl[i * ldp + tx] = acc;
        }
        __syncthreads();
      }
      // ---- Hn_k, c_k out; Pi_k = sym(.), its change against the last sweep
      double dmax = 0.0, vabs = 0.0;
      if (tx < nx) {
        double* Nk = Hn + (size_t)k * nx * nx;
        for (int j = ty; j < nx; j += rs) Nk[j * nx + tx] = j < c ? HnC[j * ldp + tx] : 0.0;
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
      if (tid == 0) cnt[k] = c;
      dmax = lqr_wave_max(dmax); vabs = lqr_wave_max(vabs);
      if (lane == 0) { red[wv] = dmax; red[4 + wv] = vabs; }
      __syncthreads();
      dmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
      vabs = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
      { double* t_ = HnN; HnN = HnC; HnC = t_; }
      cn = c;
      if (!(dmax < INFINITY)) { status = LQR_NONFINITE; rel = INFINITY; break; }
      rel = fmax(rel, dmax / fmax(1.0, vabs));
    }
    if (status != LQR_MAXSWEEPS) break;
    sweeps = sw + 1;
    if (rel <= tol && !changed) status = LQR_OK;
  }
  if (status >= LQR_SINGULAR) sweeps += 1;                                   // the sweep that failed counts
  double* o = info + b * LQR_CTG_INFO;
  if (tid == 0) {
    o[0] = status; o[1] = sweeps; o[2] = rel; o[3] = pmin; o[4] = pmax; o[5] = (status <= LQR_MAXSWEEPS) ? posdef : 0.0;
    o[6] = (status <= LQR_MAXSWEEPS) ? posdef_path : 0.0; o[7] = 0.0; o[8] = csum; o[9] = cmax; o[10] = accmin; o[11] = rejmax;
  }
  if (status >= LQR_SINGULAR) {                                              // no closed loop to speak of
    if (Phig) for (int e = tid; e < nx * nx; e += LQR_NT) Phig[b * nx * nx + e] = qnan;
    return;
  }
  // ---- monodromy and feasibility.  Acl and K_k in the Hb buffer, Phi ping-pong between the Pi and W buffers, [Jx - Ju K_k; Hn_{k+1} Acl] in C0, Pz_k in C1
  __syncthreads();
  double* F = Pl; double* Fn = Wl; double* Acl = Hl; double* Kl = Hl + nx * ldp;
  double feas = 0.0;
  {
    const int c0 = cnt[0];
    if (tx < nx) for (int r = ty; r < c0; r += rs) HnN[r * ldp + tx] = Hn[r * nx + tx];
    __syncthreads();
    if (tx < nx) for (int r = ty; r < nx; r += rs) {
      double acc = (r == tx) ? 1.0 : 0.0;
      for (int j = 0; j < c0; ++j) acc = fma(-HnN[j * ldp + r], HnN[j * ldp + tx], acc);
      F[r * ldp + tx] = acc;
    }
    __syncthreads();
  }
  for (int k = 0; k < p; ++k) {
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Kk = K + (size_t)k * mb * nx;
    const double* Jk = J + (size_t)k * nr * n;
    const int kn = (k + 1) % p;
    const int rk = max(0, min(nr, ng + (ncnt ? ncnt[k] : 0))), ck = cnt[k], cq = cnt[kn];
    if (tx < n) for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
    if (tx < nx) {
      for (int r = ty; r < mb; r += rs) Kl[r * nx + tx] = Kk[r * nx + tx];
      for (int r = ty; r < ck; r += rs) HnN[r * ldp + tx] = Hn[(size_t)k * nx * nx + r * nx + tx];
      for (int r = ty; r < cq; r += rs) HnC[r * ldp + tx] = Hn[(size_t)kn * nx * nx + r * nx + tx];
    }
    __syncthreads();
    if (tx < nx) {
      for (int j = ty; j < rk; j += rs) {
        double acc = Jk[j * n + tx];
        for (int r = 0; r < mb; ++r) acc = fma(-Jk[j * n + nx + r], Kl[r * nx + tx], acc);
        C0[j * ldc + tx] = acc;
      }
      for (int i = ty; i < nx; i += rs) {
        double acc = El[i * ld + tx];
        for (int r = 0; r < mb; ++r) acc = fma(-El[i * ld + nx + r], Kl[r * nx + tx], acc);
        Acl[i * ldp + tx] = acc;
        double pz = (i == tx) ? 1.0 : 0.0;
        for (int j = 0; j < ck; ++j) pz = fma(-HnN[j * ldp + i], HnN[j * ldp + tx], pz);
        C1[i * ldc + tx] = pz;
      }
    }
    __syncthreads();
    if (tx < nx) {
      for (int i = ty; i < nx; i += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(Acl[i * ldp + s], F[s * ldp + tx], acc);
        Fn[i * ldp + tx] = acc;
      }
      for (int j = ty; j < cq; j += rs) {
        double acc = 0.0;
        for (int s = 0; s < nx; ++s) acc = fma(HnC[j * ldp + s], Acl[s * ldp + tx], acc);
        C0[(rk + j) * ldc + tx] = acc;
      }
    }
    __syncthreads();
    if (tx < nx) for (int i = ty; i < rk + cq; i += rs) {
      double acc = 0.0;
      for (int s = 0; s < nx; ++s) acc = fma(C0[i * ldc + s], C1[s * ldc + tx], acc);
      feas = fmax(feas, fabs(acc));
    }
    double* t_ = F; F = Fn; Fn = t_;
  }
  if (Phig && tx < nx) for (int r = ty; r < nx; r += rs) Phig[b * nx * nx + r * nx + tx] = F[r * ldp + tx];
  feas = lqr_wave_max(feas);
  if (lane == 0) red[wv] = feas;
  __syncthreads();
  if (tid == 0) o[7] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

}  // namespace tmpc
