"""Device-resident timing of the WARM-STARTED closed loop of the constrained MPC step (tunempc_amd/mpc_qp.py with warm=True, the WARM instantiations of
csrc/tmpc_mpc_qp.h) on the batch of scripts/mpc_qp_quad_timing.py: nx 24 / nu 8, p 64, 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8) with Hc from
convexify_batch, 8 initial deviations each (4096 QPs), horizon N = 6, the 16-row input box at half the largest unconstrained |u_0| of the batch, Pf = I,
steps = 16.  Four problems, each cold (the call as it was, which must not move) and warm:
        hard       the box hard;
        soft       the box soft with the L1 weight c = 0.3 max lam of each problem's hard step (some rows violated);
        terminal   terminal='constraint' beside the hard box;
        l12        the c of `soft` and Z = c (L1 + L2).
Per call: ms (median / min / max of repeated calls after warm-up, HIP events), statuses, mean iterations per step over the steps >= 1 (the steps a warm
start can change), the warm codes.  ratios: warm / cold in time and in iterations (all steps), side by side.  --tree runs the package and the built library
of another checkout; one without warm starts runs the cold calls alone, and --beside puts the figures of such runs' JSON files next to this one's (give the
parent's run twice: its own spread); --label names the build in the record.  Nothing here has a pass bar.

    python scripts/mpc_qp_warm_timing.py [--reps 5] [--batch 512] [--states 8] [--x0-scale 0.3] [--tree other/checkout] [--label 'parent commit']
                                         [--beside a.json b.json] [--out profiles/mpc_qp_warm_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--batch', type=int, default=512)
ap.add_argument('--states', type=int, default=8)
ap.add_argument('--x0-scale', type=float, default=0.3)
ap.add_argument('--tree', default=ROOT)
ap.add_argument('--beside', nargs='*', default=[])
ap.add_argument('--label', default='this checkout')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_warm_timing.json'))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
from tunempc_amd import _lib, convexifier, mpc_qp, synthetic  # noqa: E402

PROBLEMS = ('hard', 'soft', 'terminal', 'l12')


def median_ms(fn, reps, warmup=1):
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


def figures(o):
    it = o['iters'].double()
    st = o['status']
    later = it[:, :, 1:]
    out = dict(statuses={str(k): int((st == k).sum()) for k in range(4)}, iters_mean=float(it[it >= 0].mean()), iters_mean_steps_ge1=float(later[later >= 0].mean()),
               iters_max=int(it.max()), nact_steps=int((o['nact'] > 0).sum()))
    if 'warm' in o:
        out['warm_codes'] = {str(k): int((o['warm'] == k).sum()) for k in (-1, 0, 1, 2)}
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
    box = dict(D=dev(D), d=dev(np.full((nb, p, nd), umax)), Pf=dPf)
    hard = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, **box)
    lmax = hard['lam'].amax(dim=(1, 2, 3)).clamp_min(1e-3)                   # per problem
    c = (0.3 * lmax)[:, None, None].expand(nb, p, nd).contiguous()
    has_warm = hasattr(_lib, 'mpc_qp_warm_batch_device')                     # (warm is keyword-only and not in the reported signature)
    has_quad = hasattr(_lib, 'mpc_qp_quad_batch_device')
    res = dict(device=torch.cuda.get_device_name(0), library=args.label, reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, T=T, nd=nd, umax=umax, x0_scale=args.x0_scale, instances=nb * ns, warm_floor=getattr(mpc_qp, 'WARM_FLOOR', None)))
    variants = {'hard': box, 'soft': dict(box, penalty=c), 'terminal': dict(box, terminal='constraint')}
    if has_quad:
        variants['l12'] = dict(box, penalty=c, penalty2=c.clone())
    for name, kw in variants.items():
        res[name] = {}
        for mode in ('cold', 'warm') if has_warm else ('cold',):
            extra = dict(warm=True) if mode == 'warm' else {}
            loop = lambda kw=kw, extra=extra: mpc_qp.mpc_closed_loop_batch(dA, dB, dH, dX0, N, T, return_traj=False, **kw, **extra)
            res[name][mode] = figures(loop())
            res[name][mode]['loop_ms'] = median_ms(loop, args.reps)
        print(name, json.dumps(res[name]), flush=True)
    if has_warm:
        res['ratios'] = {k: dict(time_warm_over_cold=res[k]['warm']['loop_ms']['median'] / res[k]['cold']['loop_ms']['median'],
                                 iters_warm_over_cold=res[k]['warm']['iters_mean'] / res[k]['cold']['iters_mean'],
                                 iters_warm_over_cold_steps_ge1=res[k]['warm']['iters_mean_steps_ge1'] / res[k]['cold']['iters_mean_steps_ge1']) for k in variants}
    for i, path in enumerate(args.beside):
        with open(path) as fi:
            other = json.load(fi)
        names = [k for k in variants if k in other]
        res['beside_%d' % i] = dict({k: other[k]['cold'] for k in names}, library=other['library'])
        res.setdefault('ratios', {})['cold_against_beside_%d' % i] = {k: res[k]['cold']['loop_ms']['median'] / other[k]['cold']['loop_ms']['median'] for k in names}
    print(json.dumps(res.get('ratios', {})), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fo:
        json.dump(res, fo, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
