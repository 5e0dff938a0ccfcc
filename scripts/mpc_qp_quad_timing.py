"""Device-resident timing of the MPC step and closed loop with QUADRATIC slack penalties (tunempc_amd/mpc_qp.py with penalty2=, the QUAD instantiations of
csrc/tmpc_mpc_qp.h) on the batch of scripts/mpc_qp_affine_timing.py: nx 24 / nu 8, p 64, 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8) with Hc
from convexify_batch, 8 initial deviations each (4096 QPs), horizon N = 6, the 16-row input box at half the largest unconstrained |u_0| of the batch, Pf = I.
  (1) the calls without new arguments, which must not move:
        plain      the box hard (the hard kernel);
        terminal   terminal='constraint' (the EQ kernel);
        soft       the box soft with the L1 weight c = 0.3 max lam of each problem's hard step (the SOFT kernel; some rows violated);
  (2) the new calls on the same batch:
        quad_pure  c = 0, Z = 1e2 max lam (pure quadratic: one pair per row);
        quad_l12   the c of `soft` and Z = c (L1 + L2: two pairs per row).
T = 1 and T = 16: ms per call (median / min / max of repeated calls after warm-up, HIP events), iterations per QP, statuses.  --tree runs the package and the
built library of another checkout (the cases from this one); a checkout without penalty2 runs (1) alone, and --beside puts the figures of such runs' JSON
files next to this one's (give the parent's run twice: its own spread); --label names the build in the record.  Nothing here has a pass bar.

    python scripts/mpc_qp_quad_timing.py [--reps 7] [--batch 512] [--states 8] [--x0-scale 0.3] [--tree other/checkout] [--label 'parent commit']
                                         [--beside a.json b.json] [--out profiles/mpc_qp_quad_timing.json]
"""
import argparse
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
ap.add_argument('--beside', nargs='*', default=[])
ap.add_argument('--label', default='this checkout')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_quad_timing.json'))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from tunempc_amd import _lib, convexifier, mpc_qp, synthetic  # noqa: E402

OLD = ('plain', 'terminal', 'soft')


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
    if 'nviol' in o:
        out['nviol_steps'] = int((o['nviol'] > 0).sum())
    return out


def main():
    nb, p, nx, nu, ns, N, T = args.batch, 64, 24, 8, args.states, 6, 16
    n, nd = nx + nu, 2 * nu
    A, B, H = synthetic.gen_batch(100000, nb, p, nx, nu)
    Hc = np.ascontiguousarray(convexifier.convexify_batch(A, B, H)['Hc'])
    X0 = args.x0_scale * np.random.default_rng(100004).standard_normal((nb, ns, nx))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dX0 = dev(A), dev(B), dev(Hc), dev(X0)
    dPf = dev(np.broadcast_to(np.eye(nx), (nb, p, nx, nx)))
    free = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, Pf=dPf, return_traj=False)
    umax = 0.5 * float(free['u0'].abs().max())
    D = np.zeros((nb, p, nd, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    dD, dd = dev(D), dev(np.full((nb, p, nd), umax))
    box = dict(D=dD, d=dd, Pf=dPf)
    hard = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, **box)
    lmax = hard['lam'].amax(dim=(1, 2, 3)).clamp_min(1e-3)                   # per problem
    c = (0.3 * lmax)[:, None, None].expand(nb, p, nd).contiguous()
    has_quad = hasattr(_lib, 'mpc_qp_quad_batch_device')                     # (penalty2 is keyword-only and not in the reported signature)
    res = dict(device=torch.cuda.get_device_name(0), library=args.label, reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, T=T, nd=nd, umax=umax, x0_scale=args.x0_scale, instances=nb * ns,
                          c_min=float(c.min()), c_max=float(c.max())))
    variants = {'plain': box, 'terminal': dict(box, terminal='constraint'), 'soft': dict(box, penalty=c)}
    if has_quad:
        variants['quad_pure'] = dict(box, penalty=torch.zeros_like(c), penalty2=(100.0 / 0.3) * c)
        variants['quad_l12'] = dict(box, penalty=c, penalty2=c.clone())
    for name, kw in variants.items():
        step = lambda kw=kw: mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, return_traj=False, **kw)
        loop = lambda kw=kw: mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, T, return_traj=False, **kw)
        res[name] = dict(step=figures(step(), False), loop=figures(loop(), True))
        res[name]['step_ms'] = median_ms(step, args.reps)
        res[name]['loop_ms'] = median_ms(loop, max(3, args.reps // 2), warmup=1)
        print(name, json.dumps(res[name]), flush=True)
    if has_quad:
        res['ratios'] = {k: dict(step_against_soft=res[k]['step_ms']['median'] / res['soft']['step_ms']['median'],
                                 loop_against_soft=res[k]['loop_ms']['median'] / res['soft']['loop_ms']['median'],
                                 step_iters=(res[k]['step']['iters_mean'], res['soft']['step']['iters_mean'])) for k in ('quad_pure', 'quad_l12')}
    for i, path in enumerate(args.beside):
        with open(path) as fi:
            other = json.load(fi)
        res['beside_%d' % i] = {k: other[k] for k in ('library',) + OLD}
        res.setdefault('ratios', {})['against_beside_%d' % i] = {k: dict(step=res[k]['step_ms']['median'] / other[k]['step_ms']['median'],
                                                                          loop=res[k]['loop_ms']['median'] / other[k]['loop_ms']['median']) for k in OLD}
    print(json.dumps(res.get('ratios', {})), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fo:
        json.dump(res, fo, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
