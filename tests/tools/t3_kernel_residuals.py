"""The measured figures behind the tolerances of tests/test_gpu_t3_kernels.py that are not a derived 4 gamma_m * bound (profiles/t3_kernel_residuals.txt).

Host part (no device): the residual |det(u + th du)| / (|u0 + th du0|^2 + |u1 + th du1|^2) in units of eps = 2^-53 that the fp64 numpy restatement of soc_step_eig
(tests/t3_reference.py: soc_step_eig64) leaves on the pairs of section c, per length m1 (_restatement_floor of the GPU test computes the same figure), and the
spread between tests/t3_reference.py and the oracle's fp64 cone helpers on the seeds of tests/test_t3_reference_cpu.py (ORACLE_SPREAD there).
    python tests/tools/t3_kernel_residuals.py
The device figures of that file (the ratio of the Newton-row residuals to a dense LAPACK solve, the root residuals of the kernel) are the lines
't3-newton-residual' and 'soc-step' that   pytest tests/test_gpu_t3_kernels.py -s   prints before it asserts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
import numpy as np                             # noqa: E402
import convexify_oracle as co                  # noqa: E402
import t3_reference as t3                      # noqa: E402
from test_t3_reference_cpu import _cone_point, _rel, step_pairs   # noqa: E402

EPS = 2.0 ** -53
worst = (0.0, '', 0)
for m1 in (2, 7, 11, 16, 64, 65, 67, 529, 596):
    w = (0.0, '')
    for name, u, du in step_pairs(m1):
        e = t3.soc_step_eig64(u, du)
        if e < 0:
            w = max(w, (t3.soc_root_residual(u, du, -1.0 / e) / EPS, name))
    print(f'm1 {m1:4d}: largest root residual of the fp64 restatement {w[0]:9.2f} eps ({w[1]})')
    worst = max(worst, w + (m1,))
print(f'largest: {worst[0]:.2f} eps (m1 = {worst[2]}, {worst[1]})')

for margin in (1.0, 1e-3):
    W = {}
    for m1 in (2, 7, 67, 529):
        rng = np.random.default_rng(m1)
        s, x = _cone_point(rng, m1, margin), _cone_point(rng, m1, margin)
        beta, v = t3.scaling(s, x)
        b64, v64 = co._soc_scaling(s, x)
        lam = t3.scaled_point(beta, v, x)
        r = rng.standard_normal(m1)
        dx, ds = rng.standard_normal(m1), rng.standard_normal(m1)
        cor64 = co._soc_W(b64, v64, co._soc_div(co._soc_W(b64, v64, x), co._soc_prod(co._soc_W(b64, v64, dx), co._soc_W(b64, v64, ds, inverse=True))), inverse=True)
        q = {'det': _rel(t3.det(s), co._soc_det(s)), 'beta': _rel(beta, b64), 'v': _rel(v, v64), 'W x': _rel(lam, co._soc_W(b64, v64, x)),
             'W^-1 s': _rel(lam, co._soc_W(b64, v64, s, inverse=True)), 'W^-2': _rel(t3.w2inv(beta, v), co._soc_W2inv(b64, v64)),
             'Jordan product': _rel(t3.jordan(s, r), co._soc_prod(s, r)), 'Jordan division': _rel(t3.jordan_div(s, r), co._soc_div(s, r)),
             'Mehrotra term': _rel(t3.cone_mehrotra(beta, v, lam, dx, ds), cor64)}
        for k, val in q.items():
            W[k] = max(W.get(k, 0.0), val)
    print(f'reference against the oracle, margin {margin:g} (kappa {t3.kappa(s):.4g}): ' + ', '.join(f'{k} {val:.2e}' for k, val in W.items()))
