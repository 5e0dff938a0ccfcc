// Periodic LQR gains by backward Riccati sweeps: the feedback law of a tuned scheme and the feedback-equivalence certificate
// (reference: convexifier.py:44-45 -- the LQR problems on H and on H + dH share their feedback law; examples/convex_lqr.py:52-58 checks it
// with two `dare` calls).  Per stage k of a p-periodic problem, indices mod p (include/tunempc_hip.h: tmpc_periodic_lqr_batch_*):
//     E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,  K_k = S^-1 M,  Pi_k = sym(Hb_xx - M' K_k)        (u = -K_k x)
//
// One 256-thread workgroup per problem and the WHOLE iteration in one launch (the pattern of k_ipm_small, tmpc_persist.h): every sweep, the
// convergence test, the closed-loop monodromy.  The slowly converging cases are chains of hundreds of dependent sweeps of microsecond stages
// (the reference's own LQR example: 214 sweeps at p = 1, n = 4); a launch or a host read per sweep would be all overhead.
//
// Residency: Pi (all p stages) is the output array in global memory and doubles as the state (L2-resident); the stage operands E_k, H_k -> Hb,
// Pi_{k+1} and W = Pi E live in LDS with odd leading dimensions, 131 KB at the largest shape (nx = 63, mb = 1), 26 KB at nx = 24, mb = 8.  Pi_k of a
// stage is written to LDS as well and IS the Pi_{k+1} of the next one: only the wrap-around stage k = p - 1 reads Pi back from global memory.
//
// Arithmetic: fp64 on the vector ALU.  A stage is ~2 nx n (nx + n) + 2 mb^2 n flops (1e5 at the bench shape: a fraction of a microsecond on four
// waves) cut into 6 + mb barrier-separated steps; the products have arbitrary dimensions 1 .. 64 that would be padded to 16 x 16 x 4 tiles and
// their operands moved into the MFMA fragment layout between dependent steps.  Latency of the LDS round trips decides the time, not FLOP rate.
//
// S K = M: Gauss-Jordan elimination with row pivoting on the mb x n row block [M | S] = rows nx .. n-1 of Hb (in place in LDS, ping-pong with the
// W buffer: one barrier per pivot).  S is symmetric but NOT positive definite on the way from Pi = 0 for the indefinite H this project exists for
// (R + B' Pi B has negative eigenvalues on the AWE / bench shapes), so no Cholesky.  Pivot rule: the diagonal entry when it is positive and at least
// LQR_PIV_THRESH of the column maximum (multipliers <= 1 / LQR_PIV_THRESH), else the column maximum (partial pivoting).  Elimination that never left
// a positive diagonal proves S positive definite (Sylvester) -- info[5] for the last sweep, info[6] for every sweep of the call; a positive definite S exchanges rows only if a remaining diagonal entry is
// below LQR_PIV_THRESH^2 of another, and then the flags read 0 ("not shown").  The pivots are those of LU with the same row order.
// A pivot that is zero or below LQR_SING_REL of the largest pivot of its stage ends the problem with status 2, a non-finite pivot or Pi with status 3;
// nothing of another problem is touched.
#pragma once
#include "tmpc_common.h"

namespace tmpc {

constexpr int LQR_NT = 256;                  // threads per problem
constexpr int LQR_NMAX = 64;                 // nx + mb served (TMPC_LQR_NMAX)
constexpr double LQR_PIV_THRESH = 0.1;
constexpr double LQR_SING_REL = 1e-13;
enum { LQR_OK = 0, LQR_MAXSWEEPS = 1, LQR_SINGULAR = 2, LQR_NONFINITE = 3 };

struct LqrLds { int ld, ldp, oE, oP, oW, oH, oR, total; };      // offsets in doubles
__host__ __device__ inline LqrLds lqr_lds(int nx, int mb) {
  LqrLds l;
  const int n = nx + mb, mr = nx > mb ? nx : mb;
  l.ld = n | 1; l.ldp = nx | 1;
  l.oE = 0;                     // E_k [nx x n]
  l.oP = l.oE + nx * l.ld;      // Pi_{k+1} [nx x nx], then Hb_xx - M'K, then Pi_k
  l.oW = l.oP + nx * l.ldp;     // W = Pi E [nx x n]; second buffer of the elimination [mb x n]
  l.oH = l.oW + mr * l.ld;      // Hb [n x n]
  l.oR = l.oH + n * l.ld;       // block reductions
  l.total = l.oR + 16;
  return l;
}

__device__ __forceinline__ double lqr_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// grid: nb workgroups.  cw: power of two >= n (<= 64), the column width of the thread layout (tid & (cw-1) = column, tid / cw = first row); lcw = log2 cw.
__global__ void __launch_bounds__(LQR_NT) k_periodic_lqr(int p, int nx, int mb, int lcw, const double* __restrict__ Ag, const double* __restrict__ Bg,
                                                         const double* __restrict__ Hg, const double* __restrict__ Pi0, double tol, int max_sweeps,
                                                         double* __restrict__ Kg, double* Pig, double* __restrict__ Phig, double* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int n = nx + mb;
  const LqrLds L = lqr_lds(nx, mb);
  const int ld = L.ld, ldp = L.ldp;
  double* El = lds + L.oE; double* Pl = lds + L.oP; double* Wl = lds + L.oW; double* Hl = lds + L.oH; double* red = lds + L.oR;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cw = 1 << lcw, tx = tid & (cw - 1), ty = tid >> lcw, rs = LQR_NT >> lcw;
  const size_t b = blockIdx.x;
  const double* A = Ag + b * p * nx * nx; const double* B = Bg + b * p * nx * mb; const double* H = Hg + b * p * n * n;
  double* K = Kg + b * p * mb * nx; double* Pi = Pig + b * p * nx * nx;
  const int pnn = p * nx * nx;

  for (int e = tid; e < pnn; e += LQR_NT) Pi[e] = Pi0 ? Pi0[b * pnn + e] : 0.0;
  __syncthreads();

  int status = LQR_MAXSWEEPS, sweeps = 0;
  double rel = 0.0, pmin = INFINITY, pmax = 0.0, posdef = 1.0, posdef_path = 1.0;
  for (int sw = 0; sw < max_sweeps && status == LQR_MAXSWEEPS; ++sw) {
    rel = 0.0; pmin = INFINITY; pmax = 0.0; posdef = 1.0;
    for (int k = p - 1; k >= 0; --k) {
      const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Hk = H + (size_t)k * n * n;
      // ---- operands of the stage
      if (k == p - 1) {                                                     // (every other stage finds Pi_{k+1} where the last one left it)
        const double* Pn = Pi + (size_t)((k + 1) % p) * nx * nx;
        if (tx < nx) for (int r = ty; r < nx; r += rs) Pl[r * ldp + tx] = Pn[r * nx + tx];
      }
      if (tx < n) {
        for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
        for (int r = ty; r < n; r += rs) Hl[r * ld + tx] = Hk[r * n + tx];
      }
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
      // ---- [M | S] -> [K | I]: one pivot per barrier, src -> dst
      double* src = Hl + nx * ld; double* dst = Wl;
      double spmax = 0.0;
      for (int c = 0; c < mb; ++c) {
        const int pc = nx + c;
        double v = (lane < mb - c) ? fabs(src[(c + lane) * ld + pc]) : -1.0;      // every wave finds the pivot for itself: no barrier for the search
        if (v != v) v = INFINITY;
        const double vmax = lqr_wave_max(v);
        const unsigned long long hit = __ballot(v == vmax);
        int pr = c + __ffsll((long long)hit) - 1;
        const double diag = src[c * ld + pc];
        const bool keep = diag > 0.0 && diag >= LQR_PIV_THRESH * vmax;
        if (keep) pr = c; else { posdef = 0.0; posdef_path = 0.0; }
        const double pv = src[pr * ld + pc], apv = fabs(pv);
        if (!(apv < INFINITY)) { status = LQR_NONFINITE; break; }
        if (!(apv > LQR_SING_REL * spmax)) { status = LQR_SINGULAR; pmin = fmin(pmin, apv); break; }
        spmax = fmax(spmax, apv); pmin = fmin(pmin, apv); pmax = fmax(pmax, apv);
        const double inv = 1.0 / pv;
        if (tx < n && !(tx >= nx && tx <= pc)) {                             // (the columns of S already reduced are never read again)
          const double pj = src[pr * ld + tx] * inv;
          for (int r = ty; r < mb; r += rs) {
            const int q = (r == pr) ? c : r;                                 // row pr receives what stood in row c
            dst[r * ld + tx] = (r == c) ? pj : fma(-src[q * ld + pc], pj, src[q * ld + tx]);
          }
        }
        __syncthreads();
        double* t_ = src; src = dst; dst = t_;
      }
      if (status != LQR_MAXSWEEPS) break;                                    // (uniform: every thread read the same pivots)
      // ---- K_k out; Hb_xx - M' K_k
      if (tx < nx) {
        double* Kk = K + (size_t)k * mb * nx;
        for (int r = ty; r < mb; r += rs) Kk[r * nx + tx] = src[r * ld + tx];
        for (int i = ty; i < nx; i += rs) {
          double acc = Hl[i * ld + tx];
          for (int r = 0; r < mb; ++r) acc = fma(-Hl[i * ld + nx + r], src[r * ld + tx], acc);
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
  if (tid == 0) {
    double* o = info + b * 8;
    o[0] = status; o[1] = sweeps; o[2] = rel; o[3] = pmin; o[4] = pmax; o[5] = (status <= LQR_MAXSWEEPS) ? posdef : 0.0; o[6] = (status <= LQR_MAXSWEEPS) ? posdef_path : 0.0; o[7] = 0.0;
  }
  if (!Phig) return;
  double* Phi = Phig + b * nx * nx;
  if (status >= LQR_SINGULAR) {                                              // no closed loop to speak of
    for (int e = tid; e < nx * nx; e += LQR_NT) Phi[e] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  // ---- monodromy Phi = (A_{p-1} - B_{p-1} K_{p-1}) ... (A_0 - B_0 K_0): Acl and K_k in the Hb buffer, Phi ping-pong between the Pi and W buffers
  __syncthreads();
  double* F = Pl; double* Fn = Wl; double* Acl = Hl; double* Kl = Hl + nx * ldp;
  if (tx < nx) for (int r = ty; r < nx; r += rs) F[r * ldp + tx] = (r == tx) ? 1.0 : 0.0;
  for (int k = 0; k < p; ++k) {
    const double* Ak = A + (size_t)k * nx * nx; const double* Bk = B + (size_t)k * nx * mb; const double* Kk = K + (size_t)k * mb * nx;
    if (tx < n) for (int r = ty; r < nx; r += rs) El[r * ld + tx] = tx < nx ? Ak[r * nx + tx] : Bk[r * mb + tx - nx];
    if (tx < nx) for (int r = ty; r < mb; r += rs) Kl[r * nx + tx] = Kk[r * nx + tx];
    __syncthreads();
    if (tx < nx) for (int i = ty; i < nx; i += rs) {
      double acc = El[i * ld + tx];
      for (int r = 0; r < mb; ++r) acc = fma(-El[i * ld + nx + r], Kl[r * nx + tx], acc);
      Acl[i * ldp + tx] = acc;
    }
    __syncthreads();
    if (tx < nx) for (int i = ty; i < nx; i += rs) {
      double acc = 0.0;
      for (int s = 0; s < nx; ++s) acc = fma(Acl[i * ldp + s], F[s * ldp + tx], acc);
      Fn[i * ldp + tx] = acc;
    }
    __syncthreads();
    double* t_ = F; F = Fn; Fn = t_;
  }
  if (tx < nx) for (int r = ty; r < nx; r += rs) Phi[r * nx + tx] = F[r * ldp + tx];
}

}  // namespace tmpc
