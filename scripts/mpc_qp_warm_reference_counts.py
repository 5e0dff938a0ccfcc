"""Iteration counts of the warm-started MPC step on the numpy reference (tests/mpc_qp_warm_reference.py), no GPU: for every problem of its `problems()` the
receding-horizon loop over 12 steps, cold and warm at several absolute floors and at the floor 1e-2 max(1, |d_i|) scaled per row (`rel`), summed over the steps 1 .. 11 and over the instances; the worst single-step excess of
the warm loop over the cold one; the count of retried and of failed steps; the largest distance between the warm and the cold trajectory.

    python scripts/mpc_qp_warm_reference_counts.py [--cases a,b] > profiles/mpc_qp_warm_reference_counts.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mpc_qp_warm_reference as wr  # noqa: E402

T = 12
FLOORS = (3e-2, 1e-2, 3e-3, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='')
    args = ap.parse_args()
    prs = wr.problems()
    names = [n for n in prs if not args.cases or n in args.cases.split(',')]
    print('steps 1 .. %d of a %d-step loop, iterations summed over the instances; "excess": worst single step, warm minus cold; "retried": warm code 2' % (T - 1, T))
    print('%-13s %5s | %s %8s | excess at 1e-2 | retried | failed' % ('problem', 'cold', ' '.join('%8s' % ('d=%g' % f) for f in FLOORS), 'rel 1e-2'))
    for name in names:
        cold = wr.loops(name, False, T)
        tot = lambda L: sum(int(r['iters'][1:].sum()) for rb in L for r in rb)
        row, exc, retried, failed = [], 0, 0, 0
        for f in FLOORS:
            warm = wr.loops(name, True, T, f)
            row.append(tot(warm))
            failed += sum(r['status'] != 0 for rb in warm for r in rb)
            if f == 1e-2:
                exc = max(int((w['iters'][1:] - c['iters'][1:]).max()) for wb, cb in zip(warm, cold) for w, c in zip(wb, cb))
                retried = sum(int((w['warm'] == wr.RETRIED).sum()) for wb in warm for w in wb)
                dx = max(np.abs(w['X'] - c['X']).max() for wb, cb in zip(warm, cold) for w, c in zip(wb, cb))
        rel = wr.loops(name, True, T, 1e-2, True)
        failed += sum(r['status'] != 0 for rb in rel for r in rb)
        print('%-13s %5d | %s %8d | %+14d | %7d | %6d   (warm against cold trajectories: %.1e)' % (name, tot(cold), ' '.join('%8d' % v for v in row), tot(rel), exc, retried,
                                                                                               failed, dx))


if __name__ == '__main__':
    main()
