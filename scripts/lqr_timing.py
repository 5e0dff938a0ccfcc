"""Device-resident timing of the periodic LQR kernel and of the feedback-equivalence certificate (tunempc_amd/lqr.py, csrc/tmpc_lqr.h):
  - the bench batch: 512 problems of synthetic.gen_batch(100000, ., 64, 24, 8), certificate on the Hc / P of convexify_batch,
  - c1 (tests/golden/c1_convex_lqr.npz) at batch 1: 214 dependent sweeps, the latency case,
  - c3 (tests/golden/c3_evaporation_shape.npz, its three members tiled) at batch 256.
Inputs live in HBM; HIP events around (a) the C entry alone (`entry_ms`: launch + synchronise), (b) periodic_lqr_batch (`call_ms`: plus the spectral radii
on the host) and (c) feedback_equivalence_batch (`certificate_ms`: two recursions and the comparison).  Warm-up, then the median of --reps calls.
Compared with: the numpy statement of the recursion on this host (tests/lqr_reference.py, one pass) and the convexify step of the same batch (BENCH_r06.json).
The rows leg (csrc/tmpc_lqr_rows.h) times, in the same run on the same inputs (the Hc of the bench batch), the plain entry, the rows entry with 2 + 0..3 random
rows per stage and the rows entry with room for 5 rows that no stage uses, and the certificate with rows -> profiles/lqr_rows_timing.json.
The ctg leg (--ctg; csrc/tmpc_lqr_ctg.h) times, on the Hc side of the same batch with 5 random rows at every stage, the rows entry and the constraint-to-go
entry next to each other (the rows fit the inputs, so both serve them), and the two certificates -> profiles/lqr_ctg_timing.json; nothing else is run.
The horizon leg (--horizon; csrc/tmpc_lqr_horizon.h) times, on the same inputs as the ctg leg, the finite-horizon entry from all 64 phases with terminal='cost'
at N = 16 and N = 64 interleaved with the constraint-to-go entry, and reports the time per workgroup-stage of both -> profiles/lqr_horizon_timing.json.

    python scripts/lqr_timing.py [--reps 15] [--batch 512] [--out profiles/lqr_timing.json] [--rows-out profiles/lqr_rows_timing.json] [--rows-only]
    python scripts/lqr_timing.py --ctg [--reps 15] [--batch 512] [--ctg-out profiles/lqr_ctg_timing.json]
    python scripts/lqr_timing.py --horizon [--reps 15] [--batch 512] [--horizon-out profiles/lqr_horizon_timing.json]
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
import lqr_reference as lr  # noqa: E402
from tunempc_amd import _lib, convexifier, lqr, synthetic  # noqa: E402


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


def measure(tag, A, B, H, Hc, P, reps, numpy_members):
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, H, Hc, P)]
    dA, dB, dH, dHc, dP = dev
    out = lqr.periodic_lqr_batch(dA, dB, dH)
    cert = lqr.feedback_equivalence_batch(dA, dB, dH, dHc)
    certP = lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP)
    res = dict(shape=dict(nb=int(A.shape[0]), p=int(A.shape[1]), nx=int(A.shape[2]), nu=int(B.shape[3])),
               sweeps=[int(out['sweeps'].min()), int(out['sweeps'].max())], converged=int((out['status'] == 0).sum()),
               dK_max=float(cert['dK'].max()), dK_max_from_P=float(certP['dK'].max()), rho_max=float(np.nanmax(out['rho'])),
               S_positive_definite_on_path=dict(from_zero=int((cert['posdef_H'] == 1.0).sum()), from_P=int((certP['posdef_H'] == 1.0).sum())))
    res['entry_ms'] = median_ms(lambda: _lib.periodic_lqr_batch_device(dA, dB, dH, None, 1e-13, 5000), reps)
    res['call_ms'] = median_ms(lambda: lqr.periodic_lqr_batch(dA, dB, dH), reps)
    res['certificate_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc), reps)
    res['certificate_from_P_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP), reps)
    m = min(numpy_members, A.shape[0])
    t = time.perf_counter(); lr.periodic_lqr_batch(A[:m], B[:m], H[:m]); el = time.perf_counter() - t
    res['numpy_reference_ms'] = dict(members_timed=m, ms_for_them=el * 1e3, ms_scaled_to_batch=el * 1e3 * A.shape[0] / m, note='one CPU thread, one pass')
    print(tag, json.dumps(res))
    return res


def measure_rows(A, B, H, Hc, P, reps):
    """Plain entry, rows entry (2 + 0..3 rows) and rows entry with zero rows on the Hc side of one batch, interleaved in one run; the certificate with rows."""
    import lqr_rows_reference as lrr
    nb, p, nx, _ = A.shape
    n = H.shape[2]
    J, ncnt = lrr.gen_rows(100001, nb, p, n, 2, 3)
    dA, dB, dH, dHc, dP, dJ, dn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, H, Hc, P, J, ncnt))
    zero = torch.zeros_like(dn)
    plain = lambda: _lib.periodic_lqr_batch_device(dA, dB, dHc, None, 1e-13, 5000)
    rows = lambda: _lib.periodic_lqr_rows_batch_device(dA, dB, dHc, dJ, dn, 2, None, 1e-13, 5000)
    norows = lambda: _lib.periodic_lqr_rows_batch_device(dA, dB, dHc, dJ, zero, 0, None, 1e-13, 5000)
    o_plain, o_rows, o_zero = plain(), rows(), norows()
    res = dict(shape=dict(nb=int(nb), p=int(p), nx=int(nx), nu=int(n - nx), ng=2, nc=3, mean_rows_per_stage=float(2 + ncnt.mean())),
               sweeps=dict(plain=[int(o_plain[3][:, 1].min()), int(o_plain[3][:, 1].max())], rows=[int(o_rows[4][:, 1].min()), int(o_rows[4][:, 1].max())]),
               converged=dict(plain=int((o_plain[3][:, 0] == 0).sum()), rows=int((o_rows[4][:, 0] == 0).sum())),
               zero_rows_bit_equal_to_plain=bool(all(torch.equal(a, b) for a, b in zip(o_plain[:3], o_zero[:3])) and torch.equal(o_plain[3], o_zero[4])),
               feas_max=float(o_rows[4][:, 7].max()))
    for rnd in range(2):                                     # two interleaved rounds: drift of the box shows as a difference between them
        res['round%d' % rnd] = dict(plain_entry_ms=median_ms(plain, reps), rows_entry_zero_rows_ms=median_ms(norows, reps), rows_entry_ms=median_ms(rows, reps))
    res['certificate_with_rows_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP, J=dJ, ncnt=dn, ng=2), reps)
    res['certificate_plain_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP), reps)
    print('rows leg', json.dumps(res))
    return res


def measure_ctg(A, B, H, Hc, P, reps):
    """Rows entry and constraint-to-go entry on the Hc side of one batch with 5 rows at every stage, interleaved in one run; the two certificates."""
    nb, p, nx, _ = A.shape
    n = H.shape[2]
    J = np.random.default_rng(100002).standard_normal((nb, p, 5, n))
    dA, dB, dH, dHc, dP, dJ = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, H, Hc, P, J))
    # random rows are not the rows Hc was convexified with: a member whose change per sweep stalls above the tolerance would run every timed call to
    # max_sweeps, so the leg stops at 1e-10 and bounds the sweeps; the counts are printed before anything is timed
    tol, max_sweeps = 1e-10, 200
    rows = lambda: _lib.periodic_lqr_rows_batch_device(dA, dB, dHc, dJ, None, 5, None, tol, max_sweeps)
    ctg = lambda: _lib.periodic_lqr_ctg_batch_device(dA, dB, dHc, dJ, None, 5, None, tol, 1e-9, max_sweeps)
    o_rows, o_ctg = rows(), ctg()
    print('ctg leg: sweeps rows', int(o_rows[4][:, 1].min()), int(o_rows[4][:, 1].max()), 'ctg', int(o_ctg[5][:, 1].min()), int(o_ctg[5][:, 1].max()), flush=True)
    ok = (o_rows[4][:, 0] == 0) & (o_ctg[5][:, 0] == 0)
    kmax = o_rows[0].abs().reshape(nb, -1).max(dim=1).values.clamp(min=1.0)
    res = dict(shape=dict(nb=int(nb), p=int(p), nx=int(nx), nu=int(n - nx), rows_per_stage=5), tol=tol, max_sweeps=max_sweeps,
               sweeps=dict(rows=[int(o_rows[4][:, 1].min()), int(o_rows[4][:, 1].max())], ctg=[int(o_ctg[5][:, 1].min()), int(o_ctg[5][:, 1].max())]),
               converged=dict(rows=int((o_rows[4][:, 0] == 0).sum()), ctg=int((o_ctg[5][:, 0] == 0).sum())),
               K_rel_diff_max=float((((o_rows[0] - o_ctg[0]).abs().reshape(nb, -1).max(dim=1).values / kmax)[ok]).max()) if bool(ok.any()) else None,
               ctg_counts_sum=int(o_ctg[4].sum()), feas_max=dict(rows=float(o_rows[4][:, 7].max()), ctg=float(o_ctg[5][:, 7].max())))
    for rnd in range(2):                                     # two interleaved rounds: drift of the box shows as a difference between them
        res['round%d' % rnd] = dict(rows_entry_ms=median_ms(rows, reps), ctg_entry_ms=median_ms(ctg, reps))
    res['certificate_with_rows_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP, J=dJ, ng=5, tol=tol, max_sweeps=max_sweeps), reps)
    res['certificate_state_rows_ms'] = median_ms(lambda: lqr.feedback_equivalence_batch(dA, dB, dH, dHc, P=dP, J=dJ, ng=5, tol=tol, max_sweeps=max_sweeps, state_rows=True), reps)
    print('ctg leg', json.dumps(res))
    return res


def measure_horizon(A, B, H, Hc, P, reps):
    """Finite-horizon entry (all p phases, terminal cost, N = 16 and N = 64) and constraint-to-go entry on the Hc side of one batch with 5 rows at every stage,
    interleaved in one run.  Time per workgroup-stage: the elapsed time over the stages all workgroups ran (ctg: its sweeps times p per problem, plus the p
    lighter stages of its monodromy pass counted as stages; horizon: nb * p * N), i.e. the throughput figure; `stage_chain_us` is the elapsed time over the
    stages ONE workgroup ran one after the other, the latency figure, which for the horizon entry includes waiting for a place on a compute unit."""
    nb, p, nx, _ = A.shape
    n = H.shape[2]
    J = np.random.default_rng(100002).standard_normal((nb, p, 5, n))
    dA, dB, dHc, dJ = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A, B, Hc, J))
    tol, max_sweeps = 1e-10, 200                             # (the settings of the ctg leg)
    ctg = lambda: _lib.periodic_lqr_ctg_batch_device(dA, dB, dHc, dJ, None, 5, None, tol, 1e-9, max_sweeps)
    hor = {N: (lambda N=N: _lib.horizon_lqr_batch_device(dA, dB, dHc, dJ, None, 5, N, None, 0, None, 1e-9, False)) for N in (16, 64)}
    o_ctg = ctg()
    sweeps = o_ctg[5][:, 1]
    print('horizon leg: ctg sweeps', int(sweeps.min()), int(sweeps.max()), flush=True)
    ctg_stages = float((sweeps.sum() + nb) * p)
    res = dict(shape=dict(nb=int(nb), p=int(p), nx=int(nx), nu=int(n - nx), rows_per_stage=5, phases=int(p), workgroups_horizon=int(nb * p), workgroups_ctg=int(nb)),
               terminal='cost', ctg=dict(tol=tol, max_sweeps=max_sweeps, sweeps=[int(sweeps.min()), int(sweeps.max())], converged=int((o_ctg[5][:, 0] == 0).sum())))
    for N, fn in hor.items():
        o = fn()
        print('horizon leg: N', N, 'done', int((o[6][..., 0] == 0).sum()), 'of', nb * p, flush=True)
        res['N%d' % N] = dict(done=int((o[6][..., 0] == 0).sum()), feas_max=float(o[6][..., 7].max()), counts_sum=int(o[3].sum()))
        if N == 64:                                          # a long horizon: K_0 against the periodic gain of the same problem
            res['N64']['K0_minus_periodic_K_max'] = float((o[0] - o_ctg[0]).abs().max())
        del o
    for rnd in range(2):                                     # two interleaved rounds: drift of the box shows as a difference between them
        r = dict(ctg_entry_ms=median_ms(ctg, reps))
        r['ctg_us_per_workgroup_stage'] = r['ctg_entry_ms']['median'] * 1e3 / ctg_stages
        r['ctg_stage_chain_us'] = r['ctg_entry_ms']['median'] * 1e3 / ((int(sweeps.max()) + 1) * p)
        for N, fn in hor.items():
            ms = median_ms(fn, reps)
            r['horizon_N%d_entry_ms' % N] = ms
            r['horizon_N%d_us_per_workgroup_stage' % N] = ms['median'] * 1e3 / (nb * p * N)
            r['horizon_N%d_stage_chain_us' % N] = ms['median'] * 1e3 / N
            r['horizon_N%d_over_ctg_per_workgroup_stage' % N] = r['horizon_N%d_us_per_workgroup_stage' % N] / r['ctg_us_per_workgroup_stage']
        res['round%d' % rnd] = r
    print('horizon leg', json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lqr_timing.json'))
    ap.add_argument('--rows-out', default=os.path.join(ROOT, 'profiles', 'lqr_rows_timing.json'))
    ap.add_argument('--rows-only', action='store_true', help='only the rows leg (it times the plain entry itself)')
    ap.add_argument('--ctg', action='store_true', help='only the constraint-to-go leg: rows entry against ctg entry with 5 rows per stage')
    ap.add_argument('--ctg-out', default=os.path.join(ROOT, 'profiles', 'lqr_ctg_timing.json'))
    ap.add_argument('--horizon', action='store_true', help='only the finite-horizon leg: horizon entry (all phases, N = 16 and 64) against the ctg entry')
    ap.add_argument('--horizon-out', default=os.path.join(ROOT, 'profiles', 'lqr_horizon_timing.json'))
    ap.add_argument('--kernel-only', action='store_true', help='one pass over the three inputs without timing (for a kernel trace)')
    args = ap.parse_args()
    assert args.reps >= 10 or args.kernel_only
    cases = {}
    A, B, H = synthetic.gen_batch(100000, args.batch, 64, 24, 8)
    conv, tconv = dict(Hc=H, P=A), 0.0
    if not args.kernel_only:
        t = time.perf_counter(); conv = convexifier.convexify_batch(A, B, H); tconv = (time.perf_counter() - t) * 1e3
    cases['bench batch %d x (p 64, nx 24, nu 8)' % args.batch] = (A, B, H, conv['Hc'], conv['P'], 32)
    if args.ctg:
        assert not args.kernel_only
        out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, optimal_members=int((conv['status'] == 0).sum()),
                   bench=measure_ctg(A, B, H, conv['Hc'], conv['P'], args.reps))
        os.makedirs(os.path.dirname(os.path.abspath(args.ctg_out)), exist_ok=True)
        with open(args.ctg_out, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', args.ctg_out)
        return
    if args.horizon:
        assert not args.kernel_only
        out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, optimal_members=int((conv['status'] == 0).sum()),
                   bench=measure_horizon(A, B, H, conv['Hc'], conv['P'], args.reps))
        os.makedirs(os.path.dirname(os.path.abspath(args.horizon_out)), exist_ok=True)
        with open(args.horizon_out, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', args.horizon_out)
        return
    if not args.kernel_only:
        step_ms = json.load(open(os.path.join(ROOT, 'BENCH_r06.json')))['parsed']['ms_per_step']
        rows = dict(device=torch.cuda.get_device_name(0), reps=args.reps, convexify_step_ms_BENCH_r06=step_ms, optimal_members=int((conv['status'] == 0).sum()),
                    bench=measure_rows(A, B, H, conv['Hc'], conv['P'], args.reps))
        rows['certificate_with_rows_share_of_convexify_step'] = rows['bench']['certificate_with_rows_ms']['median'] / step_ms
        os.makedirs(os.path.dirname(os.path.abspath(args.rows_out)), exist_ok=True)
        with open(args.rows_out, 'w') as f:
            json.dump(rows, f, indent=1)
        print('wrote', args.rows_out)
        if args.rows_only:
            return
    g = lr.load_golden('c1_convex_lqr')
    cases['c1 batch 1 (p 1, nx 3, nu 1)'] = (g['A'], g['B'], g['H'], g['Hc'], g['P'], 1)
    g = lr.load_golden('c3_evaporation_shape')
    tile = lambda x: np.tile(x, (86, 1, 1, 1))[:256].copy()
    cases['c3 batch 256 (p 50, nx 2, nu 2)'] = tuple(tile(g[k]) for k in ('A', 'B', 'H', 'Hc', 'P')) + (256,)
    if args.kernel_only:
        for tag, (A_, B_, H_, Hc_, P_, _) in cases.items():
            d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A_, B_, H_)]
            for _ in range(3):
                lqr.periodic_lqr_batch(*d)
        return
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps,
               compared_with=dict(convexify_step_ms_BENCH_r06=json.load(open(os.path.join(ROOT, 'BENCH_r06.json')))['parsed']['ms_per_step'],
                                  convexify_batch_host_entry_ms_this_run=tconv, optimal_members=int((conv['status'] == 0).sum())),
               cases={tag: measure(tag, *c[:5], args.reps, c[5]) for tag, c in cases.items()})
    bench = next(iter(out['cases'].values()))
    out['certificate_share_of_convexify_step'] = bench['certificate_ms']['median'] / out['compared_with']['convexify_step_ms_BENCH_r06']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out, 'certificate / convexify step = %.4f' % out['certificate_share_of_convexify_step'])


if __name__ == '__main__':
    main()
