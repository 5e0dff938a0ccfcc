"""Device-resident timing of the MPC step and closed loop with SOFT rows (tunempc_amd/mpc_qp.py with penalty=, the SOFT instantiation of csrc/tmpc_mpc_qp.h) with
the method and the batch of scripts/mpc_qp_timing.py: nx 24 / nu 8, p 64, 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8) with Hc from
convexify_batch, 8 initial deviations each, horizon N = 16, the 16-row input box at half the largest unconstrained |u_0| of the batch.
  - the soft entry with the whole box soft at f = 1e3 (the reference's factor: the hard solution) and f = 0.3 (rows violated), penalty = f x the largest multiplier
    of the hard solution of the batch, T = 1 and T = 16: ms per call (median / min / max of repeated calls after warm-up, HIP events), iterations per QP, statuses;
  - two baselines, neither of which runs code of the soft path: the same box hard through the entry without penalty, and the lifted problem (the slack as a
    pseudo-control, the reference's form: n = 48 with 32 rows) through the entry without penalty.
Nothing here has a pass bar.

    python scripts/mpc_qp_soft_timing.py [--reps 7] [--batch 512] [--states 8] [--out profiles/mpc_qp_soft_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tunempc_amd import convexifier, mpc_qp, synthetic  # noqa: E402


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


def figures(o, loop):
    it = (o['iters'] if loop else o['iters_total']).double()
    st = o['status']
    return dict(statuses={str(k): int((st == k).sum()) for k in range(4)}, iters_mean=float(it[it >= 0].mean()), iters_max=int(it.max()),
                nact_steps=int((o['nact'] > 0).sum()), nviol_steps=int((o['nviol'] > 0).sum()) if 'nviol' in o else 0, hres_max=float(o['hres'][st == 0].max()) if bool((st == 0).any()) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--states', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_soft_timing.json'))
    args = ap.parse_args()
    nb, p, nx, nu, ns, N, T = args.batch, 64, 24, 8, args.states, 16, 16
    n, nd = nx + nu, 2 * nu
    A, B, H = synthetic.gen_batch(100000, nb, p, nx, nu)
    Hc = np.ascontiguousarray(convexifier.convexify_batch(A, B, H)['Hc'])
    X0 = np.random.default_rng(100004).standard_normal((nb, ns, nx))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dX0 = dev(A), dev(B), dev(Hc), dev(X0)
    free = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, return_traj=False)
    umax = 0.5 * float(free['u0'].abs().max())
    D = np.zeros((nb, p, nd, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    dD, dd = dev(D), dev(np.full((nb, p, nd), umax))
    hard1 = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, D=dD, d=dd)
    lam_max = float(hard1['lam'][hard1['status'] == 0].max())
    # the lifted problem: inputs [u; e], rows [D -I] [x; u; e] <= d and -e <= 0, cost c' e, zero Hessian and zero columns of B on e
    nl = n + nd
    Bl = np.zeros((nb, p, nx, nu + nd)); Bl[..., :nu] = B
    Hl = np.zeros((nb, p, nl, nl)); Hl[:, :, :n, :n] = Hc
    Dl = np.zeros((nb, p, 2 * nd, nl)); Dl[:, :, :nd, :n] = D; Dl[:, :, :nd, n:] = -np.eye(nd); Dl[:, :, nd:, n:] = -np.eye(nd)
    dl = np.zeros((nb, p, 2 * nd)); dl[:, :, :nd] = umax
    dBl, dHl, dDl, ddl = dev(Bl), dev(Hl), dev(Dl), dev(dl)
    del Bl, Hl, Dl
    lay_h, lay_s, lay_l = mpc_qp.lds_layout(nx, nu, nd), mpc_qp.lds_layout(nx, nu, nd, soft=True), mpc_qp.lds_layout(nx, nu + nd, 2 * nd)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, T=T, nd=nd, umax=umax, lam_max_hard=lam_max, instances=nb * ns, lifted=dict(n=nl, rows=2 * nd),
                          lds_bytes=dict(hard=lay_h['bytes'], soft=lay_s['bytes'], lifted=lay_l['bytes']),
                          workspace_bytes_per_slot=dict(hard=8 * lay_h['ws_doubles'](N), soft=8 * lay_s['ws_doubles'](N), lifted=8 * lay_l['ws_doubles'](N)),
                          vgprs=dict(hard=221, soft=246), scratch_bytes=0))
    calls = {'hard': (lambda steps: (lambda: (mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, D=dD, d=dd, return_traj=False) if steps == 1 else
                                              mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, steps, D=dD, d=dd, return_traj=False))))}
    for f in (1e3, 0.3):
        pen = dev(np.full((nb, p, nd), f * lam_max))
        ql = np.zeros((nb, p, nl)); ql[..., n:] = f * lam_max
        dql = dev(ql)
        calls['soft_f%g' % f] = (lambda steps, pen=pen: (lambda: (mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, D=dD, d=dd, penalty=pen, return_traj=False) if steps == 1 else
                                                                  mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, steps, D=dD, d=dd, penalty=pen, return_traj=False))))
        calls['lifted_f%g' % f] = (lambda steps, q=dql: (lambda: (mpc_qp.mpc_qp_batch(dA, dBl, dHl, dX0, N, D=dDl, d=ddl, q=q, return_traj=False) if steps == 1 else
                                                                  mpc_qp.mpc_closed_loop_batch(dA, dBl, dHl, dX0, N, steps, D=dDl, d=ddl, q=q, return_traj=False))))
    for name, mk in calls.items():
        step, loop = mk(1), mk(T)
        o1, oT = step(), loop()
        res[name] = dict(step=figures(o1, False), loop=figures(oT, True))
        res[name]['step_ms'] = median_ms(step, args.reps)
        res[name]['loop_ms'] = median_ms(loop, max(3, args.reps // 2), warmup=1)
        if name.startswith('soft') or name.startswith('lifted'):
            f = name.split('_f')[1]
            if name.startswith('soft'):
                res[name]['u0'] = o1['u0']
            else:
                res[name]['u0_against_soft'] = float((o1['u0'][..., :nu] - res['soft_f' + f]['u0']).abs().max())
        print(name, json.dumps({k: v for k, v in res[name].items() if k != 'u0'}), flush=True)
    for f in ('1000', '0.3'):
        del res['soft_f' + f]['u0']
    h = res['hard']
    res['ratios'] = {k: dict(step_against_hard=res[k]['step_ms']['median'] / h['step_ms']['median'], loop_against_hard=res[k]['loop_ms']['median'] / h['loop_ms']['median'])
                     for k in res if k.startswith('soft') or k.startswith('lifted')}
    for f in ('1000', '0.3'):
        res['ratios']['soft_f' + f]['step_against_lifted'] = res['soft_f' + f]['step_ms']['median'] / res['lifted_f' + f]['step_ms']['median']
        res['ratios']['soft_f' + f]['loop_against_lifted'] = res['soft_f' + f]['loop_ms']['median'] / res['lifted_f' + f]['loop_ms']['median']
    print(json.dumps(res['ratios']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fo:
        json.dump(res, fo, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
