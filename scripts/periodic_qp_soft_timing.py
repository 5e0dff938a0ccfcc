"""Device-resident timing of the periodic QP with soft rows at the batch of scripts/periodic_qp_timing.py: 4096 problems, nx 24 / nu 8, p = N = 6, the 16-row
input box at half the largest input of each problem's orbit without rows.
  - the hard call (no penalty: the existing entry, k_periodic_qp<false>): ms per call (median / min / max, HIP events), iterations per problem;
  - the soft call at c of half the hard multipliers (1 on the rows whose hard multiplier is zero) and the pure-quadratic call (Z = 5 on every row), with
    their iterations per problem: recorded, no threshold.
--hard-only times the hard call alone; it uses nothing but the existing entry, so the same file runs at the parent commit.  --baseline A.json B.json
reads two such runs of the parent and records whether this commit's hard call lies within their spread widened by 1 %.

    python scripts/periodic_qp_soft_timing.py [--reps 7] [--batch 4096] [--hard-only] [--baseline A.json B.json] [--out profiles/periodic_qp_soft_timing.json]
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
from tunempc_amd import periodic_qp  # noqa: E402
from mpc_qp_timing import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--hard-only', action='store_true')
    ap.add_argument('--baseline', nargs=2, default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'periodic_qp_soft_timing.json'))
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
    hard = lambda: periodic_qp.periodic_qp_batch(dA, dB, dH, q=dq, offset=dc, D=dD, d=dd)
    o = hard()
    ok = o['status'] == 0

    def figures(r):
        good = r['status'] == 0
        return dict(converged=int(good.sum()), statuses=sorted(set(r['status'].tolist())), iters_mean=float(r['iters'].double().mean()), iters_max=int(r['iters'].max()))
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, shape=dict(nb=nb, p=p, N=p, nx=nx, nu=nu, nd=2 * nu, ne=0), hard=figures(o))
    res['hard_ms'] = median_ms(hard, args.reps)
    print(json.dumps(dict(hard=res['hard'], hard_ms=res['hard_ms'])), flush=True)
    if not args.hard_only:
        res['shape'].update(lds_bytes_per_workgroup=periodic_qp.lds_bytes(nx, nu, 2 * nu, 0), soft_lds_bytes_per_workgroup=periodic_qp.lds_bytes(nx, nu, 2 * nu, 0, True),
                            soft_ws_bytes_per_slot=8 * periodic_qp.ws_doubles(nx, nu, 2 * nu, 0, p, True))
        lam = torch.where(ok[:, None, None], o['lam'], torch.zeros_like(o['lam']))      # p = N: lam [nb, N, nd] is [nb, p, nd]
        pen = torch.where(lam > 0, 0.5 * lam, torch.ones_like(lam)).contiguous()
        z5 = torch.full_like(pen, 5.0)
        soft = lambda: periodic_qp.periodic_qp_batch(dA, dB, dH, q=dq, offset=dc, D=dD, d=dd, penalty=pen)
        pure = lambda: periodic_qp.periodic_qp_batch(dA, dB, dH, q=dq, offset=dc, D=dD, d=dd, penalty2=z5)
        for name, fn in (('soft', soft), ('pure', pure)):
            r = fn()
            good = r['status'] == 0
            res[name] = dict(figures(r), nviol_mean=float(r['nviol'][good].double().mean()), emax_max=float(r['emax'][good].max()))
            res[name + '_ms'] = median_ms(fn, args.reps)
            res[name + '_over_hard'] = res[name + '_ms']['median'] / res['hard_ms']['median']
            print(json.dumps({name: res[name], name + '_ms': res[name + '_ms']}), flush=True)
    if args.baseline:
        runs = [json.load(open(f))['hard_ms'] for f in args.baseline]
        lo, hi = min(r['median'] for r in runs), max(r['median'] for r in runs)
        res['parent_hard_ms'] = runs
        res['hard_within_parent_spread_widened_by_1_percent'] = bool(res['hard_ms']['median'] <= hi * 1.01)
        res['parent_spread'] = dict(lo=lo, hi=hi, bar=hi * 1.01)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
