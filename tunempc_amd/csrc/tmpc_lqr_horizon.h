// Finite-horizon LQR gains: the first-order feedback u_0 = -K_0 x_0 of a horizon-N problem on a p-periodic model, from every starting phase k0.  One backward
// pass j = N-1 ... 0 over the stages k = (k0 + j) mod p, no convergence loop; N may be smaller than, equal to or larger than p.  The pass starts from
//   Pi_N = Pf[(k0 + N) mod p] (null: zero),  Hn_N empty (terminal cost)  or  Hn_N = I, c_N = nx (terminal constraint x_N = 0)
// and runs the stage of k_periodic_lqr_ctg (tmpc_lqr_ctg.h: stack, split with full pivoting, compression to Hn, bordered solve with the row scaling,
// projection) on a copy of that code that lives here, so that the periodic kernels stay as they are.  A terminal constraint is the constraint-to-go recursion
// started from the identity; c = nx is legal at that given stage only, a computed c_j = nx ends the (problem, phase) with status 5.
//
// Residency: grid nb x nph, one 256-thread workgroup per (problem, starting phase), the LDS layout of the ctg kernel (lqr_ctg_lds; valid for nr = 0: no stack
// rows besides the constraint-to-go, J may be null).  Pi and Hn stay in LDS from one stage to the next; E_k, H_k, J_k come from global memory per stage.
// fp64 on the vector ALU; the chain of a pass is latency-bound, the independent workgroups hide it.
//
// feas = max_j max(|(Jx - Ju K_j) Pz_j|, |Hn_{j+1} (A - B K_j) Pz_j|) is taken inside each stage, there is no second pass: the split destroys the stack, so it
// is built once more (rows of J_k from global memory, Hn_{j+1} E from LDS) into the buffer the projection has released, K_j is applied in place and the result
// meets Pz_j, which is still in the other stack buffer.
//
// Statuses: 0 done, 2 singular stage system, 3 non-finite, 5 no feasible subspace (there is no 1 and no 4).  A (problem, phase) that ends with status >= 2
// writes NaN to its K0 and Pi0, zero to Hn0, the count of the failing stage (nx for status 5) to cnt0, and NaN / -1 to the stages of Kall / cntall it did not finish.
#pragma once
#include "tmpc_lqr_ctg.h"

namespace tmpc {

enum { LQR_TERMINAL_COST = 0, LQR_TERMINAL_CONSTRAINT = 1 };

// grid: (nb, nph).  phases [nph] or null (phase = blockIdx.y; then nph = p).  cw, lcw as in k_periodic_lqr_rows.  J [nb][p][nr][n] or null when nr = 0,
// ncnt [nb][p] or null (ng rows everywhere; counts are clamped to 0 .. nr), Pf [nb][p][nx][nx] or null.
// Outputs: K0 [nb][nph][mb][nx], Pi0 [nb][nph][nx][nx], Hn0 [nb][nph][nx][nx] (rows beyond c_0 zero), cnt0 [nb][nph], info [nb][nph][12],
// Kall [nb][nph][N][mb][nx] and cntall [nb][nph][N] or null.
__global__ void __launch_bounds__(LQR_NT) k_horizon_lqr(int p, int nx, int mb, int nr, int ng, int lcw, int N, const int* __restrict__ phases, int terminal,
                                                        const double* __restrict__ Ag, const double* __restrict__ Bg, const double* __restrict__ Hg,
                                                        const double* __restrict__ Jg, const int* __restrict__ ncntg, const double* __restrict__ Pfg,
                                                        double rank_tol, double* __restrict__ K0g, double* __restrict__ Pi0g, double* __restrict__ Hn0g,
                                                        int* __restrict__ cnt0g, double* __restrict__ Kallg, int* __restrict__ cntallg,
                                                        double* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const LqrCtgLds L = lqr_ctg_lds(nx, mb, nr);
  const int ld = L.ld, ldp = L.ldp, ldc = L.ldc, nbd = L.nbd;
  double* El = lds + L.oE; double* Pl = lds + L.oP; double* Wl = lds + L.oW; double* Hl = lds + L.oH; double* red = lds + L.oR;
  double* C0 = lds + L.oC0; double* C1 = lds + L.oC1; double* HnN = lds + L.oN0; double* HnC = lds + L.oN1;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const size_t b = blockIdx.x, nph = gridDim.y, bp = b * nph + blockIdx.y;
  const int k0 = phases ? phases[blockIdx.y] : (int)blockIdx.y;
  const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* H = Hg + b * p * n * n;
  const double* J = nr > 0 ? Jg + b * p * nr * n : nullptr; const int* ncnt = ncntg ? ncntg + b * p : nullptr;
  double* K0 = K0g + bp * mb * nx; double* Pi0 = Pi0g + bp * nx * nx; double* Hn0 = Hn0g + bp * nx * nx;
  double* Kall = Kallg ? Kallg + bp * N * mb * nx : nullptr; int* cntall = cntallg ? cntallg + bp * N : nullptr;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- the start of the pass: Pi_N and Hn_N
  int cn = terminal == LQR_TERMINAL_CONSTRAINT ? nx : 0;
  if (tx < nx) {
    const double* Pn = Pfg ? Pfg + (b * p + (size_t)((k0 + N % p) % p)) * nx * nx : nullptr;
    for (int r = ty; r < nx; r += rs) {
      Pl[r * ldp + tx] = Pn ? Pn[r * nx + tx] : 0.0;
      if (cn) HnN[r * ldp + tx] = (r == tx) ? 1.0 : 0.0;
    }
  }
  __syncthreads();

  int status = LQR_OK, done = 0, csum = 0, cmax = 0, cfail = 0;
  double pmin = INFINITY, pmax = 0.0, posdef = 1.0, accmin = INFINITY, rejmax = 0.0, feas = 0.0;
  for (int j = N - 1; j >= 0; --j) {
    const int k = (k0 + j % p) % p;
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Hk = H + (size_t)k * n * n;
    const double* Jk = J ? J + (size_t)k * nr * n : nullptr;
    const int rk = max(0, min(nr, ng + (ncnt ? ncnt[k] : 0)));
    // ---- operands of the stage (Pi_{j+1}, Hn_{j+1} stand where the last stage left them)
    if (tx < n) {
      for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
      for (int r = ty; r < n; r += rs) Hl[r * ld + tx] = Hk[r * n + tx];
      for (int i = ty; i < rk; i += rs) C0[i * ldc + tx] = Jk[i * n + tx];
    }
    if (tx < nbd) for (int i = ty; i < nbd; i += rs) Hl[(n + i) * ld + n + tx] = 0.0;
    __syncthreads();
    // ---- W = Pi_{j+1} E; the constraint-to-go seen from this stage, Hn_{j+1} E, below the rows of J_k
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
        for (int i = ty; i < rk; i += rs) C1[i * ldc + tx] = Jk[i * n + tx];
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
  if (lane == 0) red[8 + wv] = feas;                                       // (slots of their own: a pass that broke off may still have readers of red[0 .. 3])
  __syncthreads();
  double* o = info + bp * LQR_CTG_INFO;
  if (tid == 0) {
    o[0] = status; o[1] = N; o[2] = done; o[3] = pmin; o[4] = pmax; o[5] = (status == LQR_OK) ? posdef : 0.0; o[6] = (status == LQR_OK) ? posdef : 0.0;
    o[7] = (status == LQR_OK) ? fmax(fmax(red[8], red[9]), fmax(red[10], red[11])) : 0.0;
    o[8] = csum; o[9] = cmax; o[10] = accmin; o[11] = rejmax;
    cnt0g[bp] = (status == LQR_OK) ? cn : cfail;
  }
  if (status != LQR_OK) {                                                  // nothing to return for this (problem, phase); the stages it did not finish
    for (int e = tid; e < mb * nx; e += LQR_NT) K0[e] = qnan;
    for (int e = tid; e < nx * nx; e += LQR_NT) { Pi0[e] = qnan; Hn0[e] = 0.0; }
    const int left = N - done;
    if (Kall) for (size_t e = tid; e < (size_t)left * mb * nx; e += LQR_NT) Kall[e] = qnan;
    if (cntall) for (int e = tid; e < left; e += LQR_NT) cntall[e] = -1;
  }
}

}  // namespace tmpc
