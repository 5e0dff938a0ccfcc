"""Device-resident timing of the closed-loop rollout kernel (tunempc_amd/closed_loop.py, csrc/tmpc_closed_loop.h) against a torch loop of the same recurrence on
the same device tensors, on the bench batch: 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8), Hc and P from convexify_batch, K the periodic gains of
the Hc side.
  - rollout: ns = 64 initial states per problem, T = p = 64 steps, both costs, trajectories returned -- the kernel: one launch; the torch loop: per step
    U = -K_k X, Z = [X; U], l = 1/2 colsum(Z o (H_k Z)), lc likewise, X <- A_k X + B_k U: batched products launched one after another;
  - monodromy: the rollout of X0 = I for p steps without costs or trajectories against the torch product Phi <- (A_k - B_k K_k) Phi.
Both legs run in ONE call, kernel and torch loop alternated in two rounds (drift of the box shows as a difference between the rounds), warmed up, HIP events
around each call, median / min / max of --reps repeats.  The share of the batch's convexify step (BENCH_r06.json) is reported as scripts/lqr_timing.py does.

    python scripts/closed_loop_timing.py [--reps 15] [--batch 512] [--states 64] [--out profiles/closed_loop_timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tunempc_amd import _lib, closed_loop, convexifier, lqr, synthetic  # noqa: E402


def median_ms(fn, reps, warmup=3):
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


def torch_rollout(A, B, K, X0, H, Hc, T):
    """The recurrence with torch on the device: X0 [nb,ns,nx] -> X [nb,T+1,nx,ns], U [nb,T,nu,ns], l, lc [nb,T,ns] (time-major, as the kernel stores them)."""
    nb, p, nx, _ = A.shape
    ns = X0.shape[1]
    X = torch.empty((nb, T + 1, nx, ns), dtype=torch.float64, device=A.device); U = torch.empty((nb, T, B.shape[3], ns), dtype=torch.float64, device=A.device)
    l = torch.empty((nb, T, ns), dtype=torch.float64, device=A.device); lc = torch.empty_like(l)
    x = X0.transpose(1, 2)
    X[:, 0] = x
    for t in range(T):
        k = t % p
        u = -(K[:, k] @ x)
        z = torch.cat([x, u], dim=1)
        U[:, t] = u
        l[:, t] = 0.5 * (z * (H[:, k] @ z)).sum(dim=1)
        lc[:, t] = 0.5 * (z * (Hc[:, k] @ z)).sum(dim=1)
        x = A[:, k] @ x + B[:, k] @ u
        X[:, t + 1] = x
    return X, U, l, lc


def torch_monodromy(A, B, K):
    nb, p, nx, _ = A.shape
    Phi = torch.eye(nx, dtype=torch.float64, device=A.device).expand(nb, nx, nx)
    for k in range(p):
        Phi = (A[:, k] - B[:, k] @ K[:, k]) @ Phi
    return Phi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--states', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'closed_loop_timing.json'))
    args = ap.parse_args()
    assert args.reps >= 10
    nb, p, nx, nu, ns = args.batch, 64, 24, 8, args.states
    A, B, H = synthetic.gen_batch(100000, nb, p, nx, nu)
    conv = convexifier.convexify_batch(A, B, H)
    X0 = np.random.default_rng(100003).standard_normal((nb, ns, nx))
    dA, dB, dH, dHc, dP, dX0 = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, H, conv['Hc'], conv['P'], X0))
    per = lqr.periodic_lqr_batch(dA, dB, dHc)
    dK = per['K']
    T = p
    lay = closed_loop.lds_layout(nx, nu, 0)
    kernel = lambda: _lib.closed_loop_batch_device(dA, dB, dK, dX0, dH, dHc, None, None, 0, None, T, 0, True)
    loop = lambda: torch_rollout(dA, dB, dK, dX0, dH, dHc, T)
    eye = torch.eye(nx, dtype=torch.float64, device=dA.device).expand(nb, nx, nx).contiguous()
    mono_kernel = lambda: _lib.closed_loop_batch_device(dA, dB, dK, eye, None, None, None, None, 0, None, p, 0, False)
    mono_loop = lambda: torch_monodromy(dA, dB, dK)
    # the two sides compute the same thing (checked before anything is timed)
    o, (tX, tU, tl, tlc) = kernel(), loop()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1.0))
    agree = dict(X=rel(o['X'], tX.permute(0, 3, 1, 2)), U=rel(o['U'], tU.permute(0, 3, 1, 2)), l=rel(o['l'], tl.transpose(1, 2)), lc=rel(o['lc'], tlc.transpose(1, 2)),
                 Phi=rel(mono_kernel()['XT'].transpose(1, 2), mono_loop()), Phi_against_periodic_entry=rel(mono_kernel()['XT'].transpose(1, 2), per['Phi']))
    cert = closed_loop.cost_equivalence_batch(dA, dB, dH, dHc, dP, dK, dX0, T)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, T=T, states_per_workgroup=lay['ts'], lds_bytes_per_workgroup=lay['bytes'],
                          workgroups_rollout=nb * -(-ns // lay['ts']), workgroups_monodromy=nb * -(-nx // lay['ts'])),
               optimal_members=int((conv['status'] == 0).sum()), converged_gains=int((per['status'] == 0).sum()), rho_max=float(np.nanmax(per['rho'])),
               rollouts_done=int((o['info'][..., 0] == 0).sum()), kernel_against_torch_loop=agree,
               certificate=dict(defect_rel_max=float(np.nanmax(cert['defect_rel'])), defect_rel_median=float(np.nanmedian(cert['defect_rel']))),
               torch_loop_launches_per_step=dict(rollout='>= 12 (3 products, 2 more for the costs, cat, elementwise, reductions, copies into the logs)', monodromy=3))
    print(json.dumps(res), flush=True)
    for rnd in range(2):                                     # two interleaved rounds: drift of the box shows as a difference between them
        r = dict(rollout_kernel_ms=median_ms(kernel, args.reps), rollout_torch_loop_ms=median_ms(loop, args.reps),
                 monodromy_kernel_ms=median_ms(mono_kernel, args.reps), monodromy_torch_loop_ms=median_ms(mono_loop, args.reps))
        r['rollout_torch_over_kernel'] = r['rollout_torch_loop_ms']['median'] / r['rollout_kernel_ms']['median']
        r['rollout_torch_over_kernel_worst_case'] = r['rollout_torch_loop_ms']['min'] / r['rollout_kernel_ms']['max']
        r['monodromy_torch_over_kernel'] = r['monodromy_torch_loop_ms']['median'] / r['monodromy_kernel_ms']['median']
        r['monodromy_torch_over_kernel_worst_case'] = r['monodromy_torch_loop_ms']['min'] / r['monodromy_kernel_ms']['max']
        r['rollout_kernel_us_per_step'] = r['rollout_kernel_ms']['median'] * 1e3 / T
        res['round%d' % rnd] = r
        print('round', rnd, json.dumps(r), flush=True)
    res['certificate_ms'] = median_ms(lambda: closed_loop.cost_equivalence_batch(dA, dB, dH, dHc, dP, dK, dX0, T), args.reps)
    step_ms = json.load(open(os.path.join(ROOT, 'BENCH_r06.json')))['parsed']['ms_per_step']
    res['compared_with'] = dict(convexify_step_ms_BENCH_r06=step_ms)
    res['rollout_share_of_convexify_step'] = res['round1']['rollout_kernel_ms']['median'] / step_ms
    res['monodromy_share_of_convexify_step'] = res['round1']['monodromy_kernel_ms']['median'] / step_ms
    res['certificate_share_of_convexify_step'] = res['certificate_ms']['median'] / step_ms
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
