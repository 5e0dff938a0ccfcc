"""Device-resident timing of the local gain of a solved MPC step (tunempc_amd.mpc_qp.mpc_qp_gain_batch, csrc/tmpc_mpc_qp_gain.h) at the bench stage shape:
p 2 / nx 24 / nu 8, 512 problems of tests/lqr_ctg_reference.gen_problem(7, ...) (its positive definite H), 8 initial deviations each = 4096 instances,
horizon N = 6, Pf = I, the 16-row input box at half the largest unconstrained |u_0| of the batch.
  - mpc_qp_batch, device entry: ms per call (median / min / max of repeated calls after warm-up, HIP events), iterations, statuses;
  - mpc_qp_gain_batch on that solution, without and with the optional outputs (Kall, cntall, dX, dU): ms per call, statuses, active rows, strict;
  - the emulation it replaces, on a share of the batch: one "problem" per instance with p = N, A / B / H of the stages copied per instance and the active rows
    gathered on the host as J, through horizon_lqr_batch.  The expansion (host gather + upload) and the pass are timed separately; the two K0 are compared.
Nothing here has a pass bar.

    python scripts/mpc_qp_gain_timing.py [--reps 7] [--batch 512] [--states 8] [--share 512] [--out profiles/mpc_qp_gain_timing.json]
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
from tunempc_amd import lqr, mpc_qp  # noqa: E402
from mpc_qp_timing import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--states', type=int, default=8)
    ap.add_argument('--share', type=int, default=512, help='instances of the emulation through horizon_lqr_batch')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpc_qp_gain_timing.json'))
    args = ap.parse_args()
    import lqr_ctg_reference as lc
    nb, p, nx, nu, ns, N = args.batch, 2, 24, 8, args.states, 6
    n = nx + nu
    A, B, H, _ = lc.gen_problem(7, nb, p, nx, nu, 0)
    Pf = np.ascontiguousarray(np.broadcast_to(np.eye(nx), (nb, p, nx, nx)))
    X0 = np.random.default_rng(100004).standard_normal((nb, ns, nx))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dPf, dX0 = dev(A), dev(B), dev(H), dev(Pf), dev(X0)
    free = mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, Pf=dPf, return_traj=False)
    umax = 0.5 * float(free['u0'].abs().max())
    D = np.zeros((nb, p, 2 * nu, n)); D[:, :, :nu, nx:] = np.eye(nu); D[:, :, nu:, nx:] = -np.eye(nu)
    d = np.full((nb, p, 2 * nu), umax)
    dD, dd = dev(D), dev(d)
    solve = lambda: mpc_qp.mpc_qp_batch(dA, dB, dH, dX0, N, Pf=dPf, D=dD, d=dd)
    sol = solve()
    gain = lambda: mpc_qp.mpc_qp_gain_batch(dA, dB, dH, sol, N, Pf=dPf, D=dD, d=dd)
    gain_all = lambda: mpc_qp.mpc_qp_gain_batch(dA, dB, dH, sol, N, Pf=dPf, D=dD, d=dd, return_all=True)
    g = gain()
    ok = g['status'] == 0
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               shape=dict(nb=nb, p=p, nx=nx, nu=nu, ns=ns, N=N, nd=2 * nu, umax=umax, instances=nb * ns, gain_lds_bytes_per_workgroup=mpc_qp.gain_lds_bytes(nx, nu, 2 * nu),
                          qp_lds_bytes_per_workgroup=mpc_qp.lds_layout(nx, nu, 2 * nu)['bytes']),
               solve=dict(converged=int((sol['status'] == 0).sum()), iters_mean=float(sol['iters_total'].double().mean())),
               gain=dict(done=int(ok.sum()), statuses=sorted(set(g['status'].flatten().tolist())), active_rows_mean=float(g['nactive'].double().sum(dim=-1).mean()),
                         active_rows_max=int(g['nactive'].sum(dim=-1).max()), instances_with_active_rows=int((g['nactive'].sum(dim=-1) > 0).sum()),
                         cnt0_max=int(g['cnt0'].max()), strict_min=float(g['strict'][ok].min()), strict_below_0p99=int((g['strict'][ok] < 0.99).sum()),
                         feas_max=float(g['feas'][ok].max())))
    print(json.dumps(res), flush=True)
    res['solve_ms'] = median_ms(solve, args.reps)
    res['gain_ms'] = median_ms(gain, args.reps)
    res['gain_with_all_outputs_ms'] = median_ms(gain_all, args.reps)
    res['gain_us_per_instance'] = res['gain_ms']['median'] * 1e3 / (nb * ns)
    res['gain_over_solve'] = res['gain_ms']['median'] / res['solve_ms']['median']
    # the emulation on a share of the batch: one problem per instance, p = N
    m = min(args.share, nb * ns)
    cls = g['cls'].reshape(nb * ns, N, 2 * nu)[:m].cpu().numpy()
    t0 = time.perf_counter()
    inst_b = np.arange(m) // ns
    ks = (np.arange(N)) % p                                                  # phase0 = 0
    Ae, Be, He = A[inst_b][:, ks], B[inst_b][:, ks], H[inst_b][:, ks]
    Pe = np.ascontiguousarray(np.broadcast_to(np.eye(nx), (m, N, nx, nx)))
    cnt = (cls == 1).sum(axis=2).astype(np.int32)
    nr = max(1, int(cnt.max()))
    Je = np.zeros((m, N, nr, n))
    for i, j in zip(*np.nonzero(cnt)):
        rows = np.flatnonzero(cls[i, j] == 1)
        Je[i, j, :len(rows)] = D[inst_b[i], ks[j]][rows]
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dAe, dBe, dHe, dPe, dJe, dcnt = dev(Ae), dev(Be), dev(He), dev(Pe), dev(Je), torch.from_numpy(cnt).cuda()
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    emu = lambda: lqr.horizon_lqr_batch(dAe, dBe, dHe, N, terminal='cost', Pf=dPe, phases=[0], J=dJe, ncnt=dcnt)
    e = emu()
    K0 = g['K0'].reshape(nb * ns, nu, nx)[:m]
    both = (e['status'][:, 0] == 0) & ok.reshape(-1)[:m]
    res['emulation'] = dict(instances=m, expanded_bytes=int(sum(x.nbytes for x in (Ae, Be, He, Pe, Je))), expansion_host_ms=1e3 * host_s, expansion_upload_ms=1e3 * upload_s,
                            rows_capacity=nr, done=int((e['status'] == 0).sum()),
                            K0_against_the_gain_pass=float(((e['K0'][:, 0] - K0)[both].abs().amax() / K0[both].abs().amax().clamp(min=1.0)) if bool(both.any()) else 0.0),
                            pass_ms=median_ms(emu, args.reps))
    res['emulation']['pass_us_per_instance'] = res['emulation']['pass_ms']['median'] * 1e3 / m
    res['emulation']['expansion_us_per_instance'] = 1e3 * (res['emulation']['expansion_host_ms'] + res['emulation']['expansion_upload_ms']) / m
    print(json.dumps({k: res[k] for k in ('solve_ms', 'gain_ms', 'gain_with_all_outputs_ms', 'gain_us_per_instance', 'gain_over_solve', 'emulation')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
