"""Round 7, oracle-first check of the single-precision triangular solves: the numpy oracle (oracle/convexify_oracle.py) with the block factorisation of the
HKM Schur matrix replaced, while mu / max(1, |tau|) > switch in the main phase, by the scheme of k_cr_trsm_dma_f32 + k_cr_update_dma_f32:
  * block Cholesky L_k of every diagonal block in fp64 (pivots as before);
  * O = E L^-T in float32 from float32 roundings of L and E (LAPACK strtrs on float32 copies);
  * the Schur-complement updates D -= O O', fill = -F O' from the float32 O with float32 accumulation, subtracted from / stored into fp64;
  * the substitutions read the float32 O (as the product's k_cr_fwd_off / k_cr_bwd do in such iterations).
A Cholesky that fails on the blocks updated this way counts as a pivot failure: that factorisation is repeated in fp64 and the member stays fp64 from then on
(the product's frozen-pivot fallback, k_ctrl_c).  Reported per switch value against the all-fp64 run of the same problems: iterations, float32 factorisations per
problem, pivot failures, worst / median relative Frobenius distance of Hc, worst relative error of kappa, members not Optimal.

usage: python tests/tools/fp32_trsm_probe.py nprob [p nx mb [workers]]"""
import os
import sys

for _v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):
    os.environ.setdefault(_v, '1')
import multiprocessing as mp  # noqa: E402

import numpy as np  # noqa: E402
import scipy.linalg as sla  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
import convexify_oracle as co  # noqa: E402


def make_cls(trace, switch, count):
    f32 = np.float32

    class CholTrsm32(co._CyclicBlockChol):
        def __init__(self, D, C):
            t = trace[-1]
            self.low = switch > 0.0 and not count['off'] and t['phase'] == 0 and t['mu'] > switch * max(1.0, abs(t['tau']))
            if self.low:
                try:
                    p, d, _ = D.shape
                    self.p, self.d, self.shift = p, d, 0.0
                    self._factor32(D, C)
                    count['f32'] += 1
                    return
                except np.linalg.LinAlgError:
                    count['fail'] += 1; count['off'] = True; self.low = False
            super().__init__(D, C)

        def _factor32(self, D, C):
            p, d = self.p, self.d
            if p <= 2:
                raise ValueError('p <= 2: not probed')
            tr = lambda L, E: sla.solve_triangular(L.astype(f32), E.astype(f32).T, lower=True, check_finite=False).T          # E L^-T in float32
            Lkk = np.zeros((p, d, d)); O = np.zeros((p, d, d)); F = np.zeros((p, d, d))
            Dw = D.copy()
            Fpre = C[p - 1].copy()
            for k in range(p - 1):
                Lkk[k] = np.linalg.cholesky(Dw[k])
                sub = C[k].T.copy()
                if k == p - 2:
                    o = tr(Lkk[k], sub + Fpre)
                    assert o.dtype == f32
                    O[k] = o
                    Dw[p - 1] -= (o @ o.T).astype(np.float64)
                else:
                    o = tr(Lkk[k], sub); f = tr(Lkk[k], Fpre)
                    assert o.dtype == f32 and f.dtype == f32
                    O[k] = o; F[k] = f
                    Dw[k + 1] -= (o @ o.T).astype(np.float64)
                    Dw[p - 1] -= (f @ f.T).astype(np.float64)
                    Fpre = -(f @ o.T).astype(np.float64)
            Lkk[p - 1] = np.linalg.cholesky(Dw[p - 1])
            self.Lkk, self.O, self.F = Lkk, O, F            # O, F: float32 values (the substitutions read the float32 copies)
    return CholTrsm32


def run_one(args):
    seed, p, nx, mb, switch = args
    from tunempc_amd import synthetic
    A, B, H = synthetic.gen_batch(seed, 1, p, nx, mb)
    A, B, H = A[0], B[0], co.symmetrize(H[0])
    trace = []
    count = dict(f32=0, fail=0, off=False)
    r = co.sdp_step1(A, B, H, dict(_chol_cls=make_cls(trace, switch, count)), trace=trace)
    Hc = H + co.symmetrize(co.calH(A, B, r['P']))
    return dict(Hc=Hc, kappa=r['kappa'], iters=r['iters'], ok=r['ipm_status'] == 'optimal', f32=count['f32'], fail=count['fail'])


def main():
    nprob = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    p, nx, mb = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (64, 24, 8)
    workers = int(sys.argv[5]) if len(sys.argv) > 5 else (os.cpu_count() or 1)
    switches = (0.0, 3e-5, 1e-5)
    jobs = [(100000 + b, p, nx, mb, sw) for sw in switches for b in range(nprob)]
    with mp.Pool(workers) as pool:
        out = pool.map(run_one, jobs, chunksize=1)
    res = {sw: out[i * nprob:(i + 1) * nprob] for i, sw in enumerate(switches)}
    base = res[0.0]
    print(f'# {nprob} problems of the bench generator (tunempc_amd.synthetic, seeds 100000 ..), p={p} nx={nx} m={mb}; numpy oracle; float32 triangular solves + float32 updates')
    print('#   while mu / max(1, |tau|) > switch (main phase), fp64 block Cholesky.  columns: iterations mean (max) and members with more iterations than fp64,')
    print('#   float32 factorisations per problem, pivot failures, worst / median rel. Frobenius distance of Hc to the all-fp64 answer, worst |kappa / kappa64 - 1|, not Optimal')
    for sw in switches:
        r = res[sw]
        it = np.array([q['iters'] for q in r]); it0 = np.array([q['iters'] for q in base])
        e = np.array([np.linalg.norm(q['Hc'] - q0['Hc']) / np.linalg.norm(q0['Hc']) for q, q0 in zip(r, base)])
        dk = max(abs(q['kappa'] / q0['kappa'] - 1.0) for q, q0 in zip(r, base))
        print(f'switch {sw:7.1e}: iterations {it.mean():6.2f} ({it.max()}) more {int((it > it0).sum())}  fp32 {np.mean([q["f32"] for q in r]):5.2f}  '
              f'pivot failures {sum(q["fail"] for q in r)}  dHc worst {e.max():.1e} median {np.median(e):.1e}  dkappa {dk:.1e}  not optimal {sum(not q["ok"] for q in r)}', flush=True)


if __name__ == '__main__':
    main()
