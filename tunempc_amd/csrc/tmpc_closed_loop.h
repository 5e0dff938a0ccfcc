// Closed-loop rollouts of a phase-indexed feedback law u = -K_k x on a p-periodic model: the forward counterpart of k_horizon_lqr (the LQ content of the
// reference's closed_loop_tools.closed_loop_sim).  A tile of TS initial states of one problem walks t = 0 ... T-1 over the stages k = (k0 + t) mod p:
//   U = -K_k X,  Z = [X; U],  l = 1/2 colsum(Z o (H_k Z)),  lc = 1/2 colsum(Z o (Hc_k Z)),  rowres = colmax|J_k Z| (first r_k = ng + ncnt_k rows),
//   subres = colmax|Hn_k X| (all nx rows; rows beyond c_k are zero),  X <- A_k X + B_k U.
// This is the first-order (LQ) loop: the active set is fixed (tmpc_mpc_qp.h serves its changes) and the plant is the linearisation.
//
// Residency: grid nb x ceil(ns / TS), one 256-thread workgroup per (problem, tile); the tile [n x TS] (twice: a step reads one image and writes the next X into
// the other) stays in LDS for the whole rollout, [A_k B_k], K_k, one cost matrix (H_k, then Hc_k through the same buffer), J_k and Hn_k come from global memory
// per step.  fp64 on the vector ALU; the chain is latency-bound, the independent workgroups hide it.  Thread (rg, s) = (tid / TS, tid % TS) owns the state s and
// the matrix rows i = rg, rg + 256 / TS, ...: a wave reads a matrix entry as a broadcast (rows padded to an odd length, so the 64 / TS rows of a wave with
// TS < 64 lie in different banks) and the tile along s, conflict-free.  Four rows share one pass over the column of Z.
//
// Order of accumulation: every entry of a product is one thread's sum over j = 0, 1, ...; a column sum is the thread's sum over its rows in ascending order,
// then the sum of the 256 / TS partial sums in the order of rg.  TS is a function of (nx, nu, nr) alone (closed_loop_lds), so the numbers of a state do not
// depend on ns, on its place in the tile or on its neighbours.
//
// A state whose step t produces a non-finite number (u_t, l_t, lc_t, rowres_t, subres_t or x_{t+1}; also a non-finite x_0: step 0) ends with status 3 and
// `steps finished` = t; its entries of that step and of every later one (U, l, lc, rowres, subres from t on, X from t + 1 on, XT, sums) are NaN.  Every thread
// walks all T steps: there is no exit around a barrier, and a finished state costs its neighbours nothing but its lanes.
#pragma once
#include "tmpc_lqr_ctg.h"

namespace tmpc {

constexpr int CL_INFO = 4;                   // doubles of info per state (TMPC_CLOSED_LOOP_INFO): status, steps finished, max_t max|x_t|, reserved
constexpr int CL_PART = 6;                   // partial results per thread and step: l, lc, rowres, subres, max|x_{t+1}|, max|u_t|

struct ClosedLoopLds { int ts, lts, ldn, ldx, oE, oK, oM, oJ, oN, oZ0, oZ1, oP, oS, total; };      // offsets in doubles; ts = 0: nothing fits
// TS: 64 when two workgroups then share a CU (<= 80 KB each), else the largest power of two whose layout fits the 160 KB.
__host__ __device__ inline ClosedLoopLds closed_loop_lds(int nx, int mb, int nr) {
  ClosedLoopLds l;
  const int n = nx + mb;
  l.ldn = n | 1; l.ldx = nx | 1;
  l.oE = 0;                                  // [A_k B_k] [nx x n]
  l.oK = l.oE + nx * l.ldn;                  // K_k [mb x nx]
  l.oM = l.oK + mb * l.ldx;                  // H_k, then Hc_k [n x n]
  l.oJ = l.oM + n * l.ldn;                   // J_k [nr x n]
  l.oN = l.oJ + nr * l.ldn;                  // Hn_k [nx x nx]
  l.oP = l.oN + nx * l.ldx;                  // partial results [CL_PART][256]
  l.oS = l.oP + CL_PART * LQR_NT;            // per state: 1.0 while it runs [64]
  l.oZ0 = l.oS + 64;                         // the tile [n x TS], twice
  const long long fixed = l.oZ0, budget = LQR_LDS_BYTES / 8;
  int ts = 64;
  if (fixed + 2LL * n * 64 > budget / 2) {
    ts = 32;
    while (ts > 0 && fixed + 2LL * n * ts > budget) ts >>= 1;
  }
  l.ts = ts; l.lts = 0;
  while ((1 << l.lts) < ts) ++l.lts;
  l.oZ1 = l.oZ0 + n * ts;
  const long long total = fixed + 2LL * n * (ts > 0 ? ts : 1);
  l.total = total > 0x7fffffffLL / 8 ? 0x7fffffff / 8 : (int)total;
  return l;
}

// Four rows r0 < r1 < r2 < r3 of M (leading dimension ldm; a row index beyond nrow - 1 is clamped and its sum discarded by the caller) times the column zc of
// the tile (stride ts), each sum over j = 0 .. len - 1 in that order.
__device__ __forceinline__ void cl_dot4(const double* __restrict__ M, int ldm, int i0, int di, int nrow, const double* __restrict__ zc, int ts, int len,
                                        double& a0, double& a1, double& a2, double& a3) {
  const int last = nrow - 1;
  const double* m0 = M + (size_t)i0 * ldm;
  const double* m1 = M + (size_t)min(i0 + di, last) * ldm;
  const double* m2 = M + (size_t)min(i0 + 2 * di, last) * ldm;
  const double* m3 = M + (size_t)min(i0 + 3 * di, last) * ldm;
  a0 = 0.0; a1 = 0.0; a2 = 0.0; a3 = 0.0;
  for (int j = 0; j < len; ++j) {
    const double z = zc[j * ts];
    a0 = fma(m0[j], z, a0); a1 = fma(m1[j], z, a1); a2 = fma(m2[j], z, a2); a3 = fma(m3[j], z, a3);
  }
}

__device__ __forceinline__ double cl_absmax(double m, double a) {      // max that keeps a NaN: it becomes inf
  a = fabs(a);
  if (a != a) a = INFINITY;
  return fmax(m, a);
}

// 1/2 z' M z over the rows of this thread: sum_i z_i (M z)_i, i = rg, rg + nrg, ... in ascending order.
__device__ __forceinline__ double cl_quad(const double* __restrict__ M, int ldm, int n, int rg, int nrg, const double* __restrict__ zc, int ts) {
  double acc = 0.0;
  for (int i0 = rg; i0 < n; i0 += 4 * nrg) {
    double a0, a1, a2, a3;
    cl_dot4(M, ldm, i0, nrg, n, zc, ts, n, a0, a1, a2, a3);
    acc = fma(zc[i0 * ts], a0, acc);
    if (i0 + nrg < n) acc = fma(zc[(i0 + nrg) * ts], a1, acc);
    if (i0 + 2 * nrg < n) acc = fma(zc[(i0 + 2 * nrg) * ts], a2, acc);
    if (i0 + 3 * nrg < n) acc = fma(zc[(i0 + 3 * nrg) * ts], a3, acc);
  }
  return acc;
}

// max_i |(M z)_i| over the rows i < nrow of this thread (NaN counts as inf); the sums run over the first len entries of the column.
__device__ __forceinline__ double cl_rowmax(const double* __restrict__ M, int ldm, int nrow, int rg, int nrg, const double* __restrict__ zc, int ts, int len) {
  double m = 0.0;
  for (int i0 = rg; i0 < nrow; i0 += 4 * nrg) {
    double a0, a1, a2, a3;
    cl_dot4(M, ldm, i0, nrg, nrow, zc, ts, len, a0, a1, a2, a3);
    m = cl_absmax(m, a0);
    if (i0 + nrg < nrow) m = cl_absmax(m, a1);
    if (i0 + 2 * nrg < nrow) m = cl_absmax(m, a2);
    if (i0 + 3 * nrg < nrow) m = cl_absmax(m, a3);
  }
  return m;
}

// rows x cols doubles from global memory (dense) into LDS with leading dimension ld
__device__ __forceinline__ void cl_fetch(double* __restrict__ dst, int ld, const double* __restrict__ src, int rows, int cols, int tid) {
  for (int e = tid; e < rows * cols; e += LQR_NT) {
    const int r = e / cols;
    dst[r * ld + e - r * cols] = src[e];
  }
}

// grid: (nb, ceil(ns / TS)).  A [nb][p][nx][nx], B [nb][p][nx][mb], K [nb][p][mb][nx], X0 [nb][ns][nx]; H, Hc [nb][p][n][n] or null; J [nb][p][nr][n] or null
// (then nr = 0), ncnt [nb][p] or null (ng rows everywhere; counts are clamped to 0 .. nr); Hn [nb][p][nx][nx] or null.
// Outputs, time-major so that a tile's stores of one step are contiguous: X [nb][T+1][ns][nx], U [nb][T][ns][mb], l, lc, rowres, subres [nb][T][ns], sums
// [nb][ns][2] (sum_t l, sum_t lc in the order of t), each or null; XT [nb][ns][nx], info [nb][ns][CL_INFO].
__global__ void __launch_bounds__(LQR_NT) k_closed_loop(int p, int nx, int mb, int nr, int ng, int ns, int T, int k0, const double* __restrict__ Ag,
                                                        const double* __restrict__ Bg, const double* __restrict__ Kg, const double* __restrict__ X0g,
                                                        const double* __restrict__ Hg, const double* __restrict__ Hcg, const double* __restrict__ Jg,
                                                        const int* __restrict__ ncntg, const double* __restrict__ Hng, double* __restrict__ Xg,
                                                        double* __restrict__ Ug, double* __restrict__ lg, double* __restrict__ lcg, double* __restrict__ rowg,
                                                        double* __restrict__ subg, double* __restrict__ sumg, double* __restrict__ XTg,
                                                        double* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const ClosedLoopLds L = closed_loop_lds(nx, mb, nr);
  const int ts = L.ts, ldn = L.ldn, ldx = L.ldx;
  double* El = lds + L.oE; double* Kl = lds + L.oK; double* Ml = lds + L.oM; double* Jl = lds + L.oJ; double* Nl = lds + L.oN;
  double* part = lds + L.oP; double* run = lds + L.oS;
  double* cur = lds + L.oZ0; double* nxt = lds + L.oZ1;
  const int tid = threadIdx.x, s = tid & (ts - 1), rg = tid >> L.lts, nrg = LQR_NT >> L.lts;
  const size_t b = blockIdx.x;
  const int s0 = (int)blockIdx.y * ts, nsl = min(ts, ns - s0);              // the states s0 .. s0 + nsl - 1 of this problem
  const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* K = Kg + b * p * mb * nx;
  const double* H = Hg ? Hg + b * p * n * n : nullptr; const double* Hc = Hcg ? Hcg + b * p * n * n : nullptr;
  const double* J = (Jg && nr > 0) ? Jg + b * p * nr * n : nullptr; const int* ncnt = ncntg ? ncntg + b * p : nullptr;
  const double* Hn = Hng ? Hng + b * p * nx * nx : nullptr;
  const double* M1 = H ? H : Hc;                                            // the cost matrix of the first pass; Hc follows H when both are given
  const bool two = H && Hc;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- x_0 into the tile (states beyond ns: zero; they are never written out)
  for (int e = tid; e < ts * n; e += LQR_NT) cur[e] = 0.0;
  __syncthreads();
  {
    const double* X0 = X0g + (b * ns + s0) * nx;
    for (int e = tid; e < nsl * nx; e += LQR_NT) {
      const int q = e / nx, i = e - q * nx;
      const double v = X0[e];
      cur[i * ts + q] = v;
      if (Xg) Xg[(b * (T + 1) * ns + s0) * nx + e] = v;
    }
  }
  __syncthreads();
  double xmax = 0.0, suml = 0.0, sumlc = 0.0;                               // (of the threads tid < ts: one per state)
  int done = 0;
  if (tid < ts) {
    for (int i = 0; i < nx; ++i) xmax = cl_absmax(xmax, cur[i * ts + s]);
    const bool ok = xmax < INFINITY;
    run[s] = ok ? 1.0 : 0.0;
    if (!ok) xmax = qnan;
  }

  for (int t = 0; t < T; ++t) {
    const int k = (k0 + t % p) % p;
    const int rk = J ? max(0, min(nr, ng + (ncnt ? ncnt[k] : 0))) : 0;
    // ---- operands of the step (the last readers of these buffers are behind the barrier that ended the step before)
    cl_fetch(El, ldn, A + (size_t)k * nx * nx, nx, nx, tid);
    cl_fetch(El + nx, ldn, B + (size_t)k * nx * mb, nx, mb, tid);
    cl_fetch(Kl, ldx, K + (size_t)k * mb * nx, mb, nx, tid);
    if (M1) cl_fetch(Ml, ldn, M1 + (size_t)k * n * n, n, n, tid);
    if (rk) cl_fetch(Jl, ldn, J + (size_t)k * nr * n, rk, n, tid);
    if (Hn) cl_fetch(Nl, ldx, Hn + (size_t)k * nx * nx, nx, nx, tid);
    __syncthreads();
    // ---- U = -K X into the rows nx .. n-1 of the tile
    const double* zc = cur + s;
    for (int i0 = rg; i0 < mb; i0 += 4 * nrg) {
      double a0, a1, a2, a3;
      cl_dot4(Kl, ldx, i0, nrg, mb, zc, ts, nx, a0, a1, a2, a3);
      cur[(nx + i0) * ts + s] = -a0;
      if (i0 + nrg < mb) cur[(nx + i0 + nrg) * ts + s] = -a1;
      if (i0 + 2 * nrg < mb) cur[(nx + i0 + 2 * nrg) * ts + s] = -a2;
      if (i0 + 3 * nrg < mb) cur[(nx + i0 + 3 * nrg) * ts + s] = -a3;
    }
    __syncthreads();
    // ---- the step: first cost, residuals, x_{t+1} = [A B] z into the other image
    double p1 = M1 ? cl_quad(Ml, ldn, n, rg, nrg, zc, ts) : 0.0;
    const double pr = rk ? cl_rowmax(Jl, ldn, rk, rg, nrg, zc, ts, n) : 0.0;
    const double pn = Hn ? cl_rowmax(Nl, ldx, nx, rg, nrg, zc, ts, nx) : 0.0;
    double px = 0.0, pu = 0.0;
    for (int i0 = rg; i0 < nx; i0 += 4 * nrg) {
      double a0, a1, a2, a3;
      cl_dot4(El, ldn, i0, nrg, nx, zc, ts, n, a0, a1, a2, a3);
      nxt[i0 * ts + s] = a0; px = cl_absmax(px, a0);
      if (i0 + nrg < nx) { nxt[(i0 + nrg) * ts + s] = a1; px = cl_absmax(px, a1); }
      if (i0 + 2 * nrg < nx) { nxt[(i0 + 2 * nrg) * ts + s] = a2; px = cl_absmax(px, a2); }
      if (i0 + 3 * nrg < nx) { nxt[(i0 + 3 * nrg) * ts + s] = a3; px = cl_absmax(px, a3); }
    }
    for (int i = nx + rg; i < n; i += nrg) pu = cl_absmax(pu, zc[i * ts]);
    part[(H ? 0 : 1) * LQR_NT + tid] = p1;
    part[2 * LQR_NT + tid] = pr; part[3 * LQR_NT + tid] = pn; part[4 * LQR_NT + tid] = px; part[5 * LQR_NT + tid] = pu;
    __syncthreads();
    if (two) {                                                              // ---- the second cost through the same buffer
      cl_fetch(Ml, ldn, Hc + (size_t)k * n * n, n, n, tid);
      __syncthreads();
      p1 = cl_quad(Ml, ldn, n, rg, nrg, zc, ts);
      part[LQR_NT + tid] = p1;
      __syncthreads();
    }
    // ---- one thread per state: the partial results in the order of rg, the verdict on the step, the scalars of the step
    if (tid < ts) {
      double vl = 0.0, vlc = 0.0, vr = 0.0, vn = 0.0, vx = 0.0, vu = 0.0;
      for (int g = 0; g < nrg; ++g) {
        const int q = g * ts + s;                                           // (= the tid of the thread (g, s))
        if (H) vl += part[q];
        if (Hc) vlc += part[LQR_NT + q];
        vr = fmax(vr, part[2 * LQR_NT + q]); vn = fmax(vn, part[3 * LQR_NT + q]);
        vx = fmax(vx, part[4 * LQR_NT + q]); vu = fmax(vu, part[5 * LQR_NT + q]);
      }
      vl *= 0.5; vlc *= 0.5;
      bool ok = run[s] > 0.0;
      ok = ok && fabs(vl) < INFINITY && fabs(vlc) < INFINITY && vr < INFINITY && vn < INFINITY && vx < INFINITY && vu < INFINITY;
      if (ok) { done = t + 1; xmax = fmax(xmax, vx); suml += vl; sumlc += vlc; }
      else { run[s] = 0.0; vl = qnan; vlc = qnan; vr = qnan; vn = qnan; }
      if (s < nsl) {
        const size_t o = (b * T + t) * ns + s0 + s;
        if (lg && H) lg[o] = vl;
        if (lcg && Hc) lcg[o] = vlc;
        if (rowg && J) rowg[o] = vr;
        if (subg && Hn) subg[o] = vn;
      }
    }
    __syncthreads();
    // ---- u_t and x_{t+1} of the tile out (NaN for a state that has ended)
    if (Ug) {
      double* Uo = Ug + ((b * T + t) * ns + s0) * mb;
      for (int e = tid; e < nsl * mb; e += LQR_NT) {
        const int q = e / mb, i = e - q * mb;
        Uo[e] = run[q] > 0.0 ? cur[(nx + i) * ts + q] : qnan;
      }
    }
    if (Xg) {
      double* Xo = Xg + ((b * (T + 1) + t + 1) * ns + s0) * nx;
      for (int e = tid; e < nsl * nx; e += LQR_NT) {
        const int q = e / nx, i = e - q * nx;
        Xo[e] = run[q] > 0.0 ? nxt[i * ts + q] : qnan;
      }
    }
    { double* t_ = cur; cur = nxt; nxt = t_; }
    // (no barrier here: the fetches of the next step write E, K, M, J, Hn, whose readers are behind the barrier above; U of the next step goes into the image
    //  that was read last before that barrier as well)
  }
  // ---- x_T, info, sums
  {
    double* Xo = XTg + (b * ns + s0) * nx;
    for (int e = tid; e < nsl * nx; e += LQR_NT) {
      const int q = e / nx, i = e - q * nx;
      Xo[e] = run[q] > 0.0 ? cur[i * ts + q] : qnan;
    }
  }
  if (tid < ts && s < nsl) {
    const bool ok = run[s] > 0.0;
    double* o = info + (b * ns + s0 + s) * CL_INFO;
    o[0] = ok ? LQR_OK : LQR_NONFINITE; o[1] = done; o[2] = xmax; o[3] = 0.0;
    if (sumg) {
      double* q = sumg + (b * ns + s0 + s) * 2;
      q[0] = (ok && H) ? suml : qnan; q[1] = (ok && Hc) ? sumlc : qnan;
    }
  }
}

}  // namespace tmpc
