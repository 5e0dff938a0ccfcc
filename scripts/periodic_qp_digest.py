"""sha256 of the raw outputs of the EXISTING periodic QP entry (tunempc_amd.periodic_qp.periodic_qp_batch without penalty / penalty2, host and device
entry) on the fixed FEASIBLE and FAILING cases of tests/periodic_qp_reference.py: the evidence that a change to csrc/tmpc_periodic_qp.h leaves the hard
entry's bits alone.  Run it at the parent commit and at the commit under test on the same GPU; the lines must be equal.  It uses nothing but the existing
entry, so the same file runs at either commit.

    python scripts/periodic_qp_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from tunempc_amd import periodic_qp  # noqa: E402

KEYS = ('X', 'U', 'lam', 'nu', 'pi', 'cost', 'hres', 'eres', 'per', 'status', 'steps', 'iters', 'mu', 'rp', 'rd', 'pivmin')


def digest(o):
    h = hashlib.sha256()
    for k in KEYS:
        v = o[k].cpu().numpy() if torch.is_tensor(o[k]) else np.asarray(o[k])
        h.update(k.encode()); h.update(str(v.dtype).encode()); h.update(str(v.shape).encode()); h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import periodic_qp_reference as pq
    lines = []
    total = hashlib.sha256()
    for case in pq.FEASIBLE + [f for f, _ in pq.FAILING]:
        c = case()
        bt = pq.batch_of(c)
        host = periodic_qp.periodic_qp_batch(**bt)
        dev = periodic_qp.periodic_qp_batch(**{k: (torch.from_numpy(v).cuda() if hasattr(v, 'shape') else v) for k, v in bt.items()})
        for entry, o in (('host', host), ('device', dev)):
            d = digest(o)
            total.update(d.encode())
            lines.append('%-12s %-6s status %d iters %2d  %s' % (c['name'], entry, int(o['status'][0]), int(o['iters'][0]), d))
    lines.append('%-12s %-6s %s' % ('all', '', total.hexdigest()))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
