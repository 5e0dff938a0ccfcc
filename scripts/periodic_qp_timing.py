"""Device-resident timing of the periodic optimal-control QP (tunempc_amd.periodic_qp.periodic_qp_batch, csrc/tmpc_periodic_qp.h) at the stage shape of
scripts/mpc_qp_gain_timing.py: nx 24 / nu 8, p = N = 6, 4096 problems of tests/periodic_qp_reference._model (seed 1000 + b), the 16-row input box at half
the largest input of each problem's orbit without rows (that orbit is computed by the same call, without D).
  - periodic_qp_batch, device entry: ms per call (median / min / max of repeated calls after warm-up, HIP events), iterations per problem, statuses;
  - a cold mpc_qp_batch of the same stage shape and horizon in the same process: the same A, B, H, q, offset, D, d, one state per problem (x_0 of the orbit),
    no terminal cost: the fixed-x_0 step that the border is measured against;
  - their ratio.
The lifted emulation through mpc_qp_batch (state [x; x_0], one extra stage, terminal rows [I -I]) is not timed: see the `lifted_emulation` entry.
Nothing here has a pass bar.

    python scripts/periodic_qp_timing.py [--reps 7] [--batch 4096] [--out profiles/periodic_qp_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from tunempc_amd import mpc_qp, periodic_qp  # noqa: E402
from mpc_qp_timing import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'periodic_qp_timing.json'))
    args = ap.parse_args()
    import periodic_qp_reference as pq
    nb, p, nx, nu = args.batch, 6, 24, 8
    n = nx + nu
    models = [pq._model(1000 + b, nx, nu, p) for b in range(nb)]
    A, B, H, q, c = (np.ascontiguousarray(np.stack([m[i] for m in models])) for i in range(5))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dq, dc = dev(A), dev(B), dev(H), dev(q), dev(c)
    free = periodic_qp.periodic_qp_batch(dA, dB, dH, q=dq, offset=dc)
    umax = 0.5 * free['U'].abs().amax(dim=(1, 2))
    D = np.zeros((nb, p, 2 * nu, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    dD = dev(D); dd = umax[:, None, None].expand(nb, p, 2 * nu).contiguous()
    orbit = lambda: periodic_qp.periodic_qp_batch(dA, dB, dH, q=dq, offset=dc, D=dD, d=dd)
    o = orbit()
    ok = o['status'] == 0
    X0 = torch.where(ok[:, None], o['X'][:, 0], torch.zeros_like(o['X'][:, 0]))[:, None].contiguous()
    step = lambda: mpc_qp.mpc_qp_batch(dA, dB, dH, X0, p, q=dq, offset=dc, D=dD, d=dd, return_traj=False)
    s = step()
    active = (o['lam'] > dd - torch.einsum('bkin,bkn->bki', dD, torch.cat([o['X'], o['U']], dim=-1)))[ok]
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               shape=dict(nb=nb, p=p, N=p, nx=nx, nu=nu, nd=2 * nu, ne=0, lds_bytes_per_workgroup=periodic_qp.lds_bytes(nx, nu, 2 * nu, 0),
                          mpc_qp_lds_bytes_per_workgroup=mpc_qp.lds_layout(nx, nu, 2 * nu, ne=0)['bytes'],
                          ws_bytes_per_slot=8 * periodic_qp.ws_doubles(nx, nu, 2 * nu, 0, p)),
               periodic=dict(converged=int(ok.sum()), statuses=sorted(set(o['status'].tolist())), iters_mean=float(o['iters'].double().mean()),
                             iters_max=int(o['iters'].max()), per_max=float(o['per'][ok].max()), hres_max=float(o['hres'][ok].max()),
                             active_rows_mean=float(active.double().sum(dim=(1, 2)).mean()), free_orbit_converged=int((free['status'] == 0).sum())),
               fixed_x0=dict(converged=int((s['status'] == 0).sum()), statuses=sorted(set(s['status'].flatten().tolist())),
                             iters_mean=float(s['iters_total'].double().mean()), iters_max=int(s['iters_total'].max())))
    print(json.dumps(res), flush=True)
    res['periodic_ms'] = median_ms(orbit, args.reps)
    res['fixed_x0_ms'] = median_ms(step, args.reps)
    res['periodic_over_fixed_x0'] = res['periodic_ms']['median'] / res['fixed_x0_ms']['median']
    res['periodic_over_fixed_x0_per_iteration'] = res['periodic_over_fixed_x0'] * res['fixed_x0']['iters_mean'] / res['periodic']['iters_mean']
    res['periodic_us_per_problem'] = res['periodic_ms']['median'] * 1e3 / nb
    res['lifted_emulation'] = ('not run: with one extra stage the lifted model needs nu = nx = 24 inputs to place [x_0; x_0], and its stage block '
                               '2 nx + nu = 72 exceeds the 64 that mpc_qp_batch serves')
    print(json.dumps({k: res[k] for k in ('periodic_ms', 'fixed_x0_ms', 'periodic_over_fixed_x0', 'periodic_over_fixed_x0_per_iteration', 'periodic_us_per_problem')}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
