"""Relative residual of the linearised primal equations after the device's pass-2 direction and after a dense fp64 LAPACK solve from the same device iterate, per
case and member of tests/test_gpu_step_kernels.py, and their ratio -- the source of NEWTON_RESIDUAL_FACTOR there (profiles/step_kernel_residuals.txt):
    python tests/tools/step_kernel_residuals.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import test_gpu_step_kernels as t

print(f'{"case":34s} {"member":>6s} {"step":>8s} {"device":>10s} {"reference":>10s} {"ratio":>9s}')
worst = {}
for prm in t.PARAMS:
    c = t.run_case(prm)
    for b, phase, chord in t.members(c):
        dev, ref = t.newton_residuals(c, b, phase)
        kind = t.step_kind(c, b, chord)
        worst[kind] = max(worst.get(kind, 0.0), dev / ref)
        print(f'{t._id(prm):34s} {b:6d} {kind:>8s} {dev:10.3e} {ref:10.3e} {dev / ref:9.3g}', flush=True)
for kind, w in sorted(worst.items()):
    print(f'largest ratio, {kind} steps: {w:.3g}')
