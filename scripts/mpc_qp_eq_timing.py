"""Device-resident timing of the MPC step and closed loop with EQUALITY rows and the TERMINAL constraint (tunempc_amd/mpc_qp.py with J=, terminal=, the EQ
instantiations of csrc/tmpc_mpc_qp.h) with the method and the instance count of scripts/mpc_qp_timing.py: nx 24 / nu 8, p 64, 512 problems of
synthetic.gen_batch(100000, ., 64, 24, 8) with Hc from convexify_batch, 8 initial deviations each (scaled by --x0-scale so that the terminal constraint is
within reach of the box), horizon N = 6, the 16-row input box at half the largest unconstrained |u_0| of the batch.  The same data through
  - plain      the call without the new rows (the launch it always was: its time must not move);
  - terminal   terminal='constraint' (x_N = 0);
  - rows       3 random homogeneous equality rows on the inputs per stage (rows that also take the state at stage 0 fix u_0 from x_0 and leave most of
               this batch infeasible under the box: 3691 of 4096 instances in a first run) plus terminal='constraint';
T = 1 and T = 16: ms per call (median / min / max of repeated calls after warm-up, HIP events), iterations per QP, statuses.  --tree runs the package and the
built library of another checkout (the cases from this one); a checkout without the keywords runs `plain` alone, and --beside puts the `plain` figures of such
a run's JSON next to this one's; --label names the build in the record.  Nothing here has a pass bar.

    python scripts/mpc_qp_eq_timing.py [--reps 7] [--batch 512] [--states 8] [--x0-scale 0.3] [--tree other/checkout] [--label 'parent commit'] [--beside other.json]
                                       [--out profiles/mpc_qp_eq_timing.json]
"""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--batch', type=int, default=512)
ap.add_argument('--states', type=int, default=8)
ap.add_argument('--x0-scale', type=float, default=0.3)
ap.add_argument('--tree', default=ROOT)
ap.add_argument('--beside', default=None)
ap.add_argument('--label', default='this checkout')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_eq_timing.json'))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
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
    out = dict(statuses={str(k): int((st == k).sum()) for k in range(4)}, iters_mean=float(it[it >= 0].mean()), iters_max=int(it.max()),
               nact_steps=int((o['nact'] > 0).sum()))
    if 'eres' in o and bool((st == 0).any()):
        out['eres_max'] = float(o['eres'][st == 0].max())
    return out


def main():
    nb, p, nx, nu, ns, N, T, ne = args.batch, 64, 24, 8, args.states, 6, 16, 3
    n, nd = nx + nu, 2 * nu
    A, B, H = synthetic.gen_batch(100000, nb, p, nx, nu)
    Hc = np.ascontiguousarray(convexifier.convexify_batch(A, B, H)['Hc'])
    X0 = args.x0_scale * np.random.default_rng(100004).standard_normal((nb, ns, nx))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dX0 = dev(A), dev(B), dev(Hc), dev(X0)
    free = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, return_traj=False)
    umax = 0.5 * float(free['u0'].abs().max())
    D = np.zeros((nb, p, nd, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    dD, dd = dev(D), dev(np.full((nb, p, nd), umax))
    rng = np.random.default_rng(100005)
    J = np.zeros((nb, p, ne, n)); J[..., nx:] = rng.standard_normal((nb, p, ne, nu))
    dJ = dev(J)
    has_eq = 'terminal' in inspect.signature(mpc_qp.mpc_qp_batch).parameters
    res = dict(device=torch.cuda.get_device_name(0), library=args.label, reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, T=T, nd=nd, ne=ne, umax=umax, x0_scale=args.x0_scale, instances=nb * ns))
    variants = {'plain': {}}
    if has_eq:
        variants.update(terminal=dict(terminal='constraint'), rows=dict(J=dJ, terminal='constraint'))
        lay = {k: mpc_qp.lds_layout(nx, nu, nd, ne=e, nt=t) for k, e, t in (('plain', None, 0), ('terminal', 0, nx), ('rows', ne, nx))}
        res['shape'].update(lds_bytes={k: v['bytes'] for k, v in lay.items()}, workspace_bytes_per_slot={k: 8 * v['ws_doubles'](N) for k, v in lay.items()})
    for name, kw in variants.items():
        step = lambda kw=kw: mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, D=dD, d=dd, return_traj=False, **kw)
        loop = lambda kw=kw: mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, T, D=dD, d=dd, return_traj=False, **kw)
        res[name] = dict(step=figures(step(), False), loop=figures(loop(), True))
        res[name]['step_ms'] = median_ms(step, args.reps)
        res[name]['loop_ms'] = median_ms(loop, max(3, args.reps // 2), warmup=1)
        print(name, json.dumps(res[name]), flush=True)
    if has_eq:
        res['ratios'] = {k: dict(step_against_plain=res[k]['step_ms']['median'] / res['plain']['step_ms']['median'],
                                 loop_against_plain=res[k]['loop_ms']['median'] / res['plain']['loop_ms']['median']) for k in ('terminal', 'rows')}
    if args.beside:
        with open(args.beside) as fi:
            other = json.load(fi)
        res['plain_beside'] = dict(library=other['library'], step=other['plain']['step'], loop=other['plain']['loop'], step_ms=other['plain']['step_ms'],
                                   loop_ms=other['plain']['loop_ms'])
        res.setdefault('ratios', {})['plain_against_beside'] = dict(step=res['plain']['step_ms']['median'] / other['plain']['step_ms']['median'],
                                                                    loop=res['plain']['loop_ms']['median'] / other['plain']['loop_ms']['median'])
    print(json.dumps(res.get('ratios', {})), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fo:
        json.dump(res, fo, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
