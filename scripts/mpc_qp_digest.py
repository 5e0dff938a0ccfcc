"""sha256 of the raw outputs (u0, X, U, lam, info) of the fixed cases of tests/mpc_qp_reference.py through mpc_qp_batch and mpc_closed_loop_batch WITHOUT penalty,
host and device entry, for comparing two builds of the library bit for bit -- the hard path of csrc/tmpc_mpc_qp.h must not move when the kernel grows:

    python scripts/mpc_qp_digest.py [--tree path/to/another/checkout]      (the package and its built library are taken from that tree; the cases from this one)
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=ROOT)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
sys.path.insert(1, os.path.join(ROOT, 'tests'))
import mpc_qp_reference as mq  # noqa: E402
from tunempc_amd import _lib, mpc_qp  # noqa: E402

print('library', _lib.library_path())
T = 7


def dig(o, keys):
    h = hashlib.sha256()
    for k in keys:
        v = o[k]
        h.update(np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v).tobytes())
    return h.hexdigest()[:16]


total = hashlib.sha256()
for case in mq.CASES + [lambda: mq.case_mixed_small(2)]:
    c = case()
    opt = dict(D=c['D'], d=c['d'], Pf=c['Pf'])
    if c['q'] is not None:
        opt['q'] = c['q']
    if c['ncnt'] is not None:
        opt['ndcnt'] = c['ncnt']
    line = []
    for entry in ('host', 'device'):
        f = (lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()) if entry == 'device' else np.ascontiguousarray
        kw = {k: f(v) for k, v in opt.items()}
        a = (f(c['A']), f(c['B']), f(c['H']), f(c['X0']), c['N'])
        line.append(dig(mpc_qp.mpc_qp_batch(*a, c['k0'], **kw), ('u0', 'X', 'U', 'lam', 'info')))
        line.append(dig(mpc_qp.mpc_closed_loop_batch(*a, T, c['k0'], **kw), ('u0', 'X', 'U', 'iters', 'nact', 'hres', 'info')))
    total.update(' '.join(line).encode())
    print('%-24s N %d  step host %s  loop host %s  step device %s  loop device %s' % (getattr(case, '__name__', 'case_mixed_small_N2'), c['N'], *line), flush=True)
print('all', total.hexdigest())
