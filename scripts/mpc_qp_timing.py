"""Device-resident timing of the inequality-constrained MPC step and closed loop (tunempc_amd/mpc_qp.py, csrc/tmpc_mpc_qp.h) at the bench stage shape:
nx 24 / nu 8, p 64, 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8) with Hc from convexify_batch, 8 initial deviations each, horizon N = 16, the
16-row input box at half the largest unconstrained |u_0| of the batch.
  - mpc_qp_batch (T = 1) and mpc_closed_loop_batch (T = 16), device entry: ms per call (median / min / max of repeated calls after warm-up, HIP events),
    iterations per QP, statuses, how many steps saturate;
  - context: the same calls without rows (nd = 0) against horizon_lqr_batch + closed_loop_batch on the same data, which is the linear law the QP reduces to;
  - the numpy reference (tests/mpc_qp_reference.py, dense interior point + polish) on a sample of instances of the same batch: seconds per instance on the host.
Nothing here has a pass bar.

    python scripts/mpc_qp_timing.py [--reps 7] [--batch 512] [--states 8] [--out profiles/mpc_qp_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from tunempc_amd import closed_loop, convexifier, lqr, mpc_qp, synthetic  # noqa: E402


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return dict(median=ts[len(ts) // 2], min=ts[0], max=ts[-1], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--states', type=int, default=8)
    ap.add_argument('--sample', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_timing.json'))
    args = ap.parse_args()
    nb, p, nx, nu, ns, N, T = args.batch, 64, 24, 8, args.states, 16, 16
    n = nx + nu
    A, B, H = synthetic.gen_batch(100000, nb, p, nx, nu)
    conv = convexifier.convexify_batch(A, B, H)
    Hc = np.ascontiguousarray(conv['Hc'])
    X0 = np.random.default_rng(100004).standard_normal((nb, ns, nx))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dX0 = dev(A), dev(B), dev(Hc), dev(X0)
    free = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, return_traj=False)
    umax = 0.5 * float(free['u0'].abs().max())
    D = np.zeros((nb, p, 2 * nu, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    d = np.full((nb, p, 2 * nu), umax)
    dD, dd = dev(D), dev(d)
    step = lambda: mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, D=dD, d=dd, return_traj=False)
    loop = lambda: mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, T, D=dD, d=dd, return_traj=False)
    step0 = lambda: mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, return_traj=False)
    loop0 = lambda: mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, T, return_traj=False)

    def law():
        g = lqr.horizon_lqr_batch(dA, dB, dH, N, terminal='cost')
        return closed_loop.closed_loop_batch(dA, dB, g['K0'], dX0, T, return_traj=False)
    o1, oT, l0, lw = step(), loop(), loop0(), law()
    lay = mpc_qp.lds_layout(nx, nu, 2 * nu)
    it1 = o1['iters_total'].double(); itT = oT['iters'].double()
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, T=T, nd=2 * nu, umax=umax, instances=nb * ns, slots=min(nb * ns, mpc_qp.SLOTS),
                          lds_bytes_per_workgroup=lay['bytes'], workspace_bytes_per_slot=8 * lay['ws_doubles'](N),
                          vgprs=221, scratch_bytes=0, waves_per_simd=2, workgroups_per_cu=2),
               step=dict(converged=int((o1['status'] == 0).sum()), iters_mean=float(it1.mean()), iters_min=int(it1.min()), iters_max=int(it1.max()),
                         saturated_instances=int((o1['nact'] > 0).sum())),
               loop=dict(converged=int((oT['status'] == 0).sum()), iters_mean=float(itT.mean()), iters_max=int(itT.max()),
                         saturated_steps=int((oT['nact'] > 0).sum()), steps=nb * ns * T),
               no_rows_against_the_law=float((l0['XT'] - lw['XT']).abs().max() / lw['XT'].abs().max().clamp(min=1.0)))
    print(json.dumps(res), flush=True)
    res['step_ms'] = median_ms(step, args.reps)
    res['loop_ms'] = median_ms(loop, max(3, args.reps // 2), warmup=1)
    res['step_no_rows_ms'] = median_ms(step0, args.reps)
    res['loop_no_rows_ms'] = median_ms(loop0, args.reps)
    res['law_gains_and_rollout_ms'] = median_ms(law, args.reps)
    res['step_us_per_instance'] = res['step_ms']['median'] * 1e3 / (nb * ns)
    res['loop_us_per_qp'] = res['loop_ms']['median'] * 1e3 / (nb * ns * T)
    res['step_us_per_instance_and_iteration'] = res['step_us_per_instance'] / max(1.0, res['step']['iters_mean'])
    # the numpy reference on a sample of the same instances (host time; dense linear algebra of order N (nx + nu) = 512)
    import mpc_qp_reference as mq
    ts, its, dis = [], [], []
    for i in range(args.sample):
        b, s = (i * 131) % nb, i % ns
        t0 = time.perf_counter()
        r = mq.solve(A[b], B[b], Hc[b], N, 0, X0[b, s], D=D[b], d=d[b])
        ts.append(time.perf_counter() - t0); its.append(int(r['a']['iters']))
        dis.append(float(np.abs(o1['u0'][b, s].cpu().numpy() - r['U'][0]).max() / max(1.0, np.abs(r['U'][0]).max())))
    res['numpy_reference'] = dict(sample=args.sample, seconds_per_instance_median=float(np.median(ts)), iters=its, u0_gpu_against_polish=dis)
    print(json.dumps({k: res[k] for k in ('step_ms', 'loop_ms', 'step_no_rows_ms', 'loop_no_rows_ms', 'law_gains_and_rollout_ms', 'numpy_reference')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
