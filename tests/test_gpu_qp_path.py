"""GPU tests of the PATH of k_mpc_qp and k_periodic_qp (csrc/tmpc_mpc_qp.h, csrc/tmpc_periodic_qp.h): the other GPU tests of these kernels check the fixed
point, and an interior-point method that centres wrongly or drops a term of its corrector still reaches it, a few iterations later.  Here every path case
of tests/qp_path_reference.py is called with max_iter = 1 .. K (K = the reference's count + 1) through both entries, and mu, rp, rd (and pivmin) of every
iterate, which the kernels write into `info` at any status, are held against the truth path of the reference:
    |f - f_ref| <= REL[class] f_ref + ABS[class],   the constants of qp_path_reference (100 x the spread of two independent means on the CPU, asserted in
    test_qp_path_cpu.py; class 'plain': no equality or terminal rows, class 'eq': with them).
Also: status 1 with iters = k before convergence, status 0 and a constant count from the converging k on; the count equal to the reference's in the class
'plain', within one in the class 'eq'; pivmin positive and non-increasing in k, and in the periodic family equal to the pivots of the restated elimination;
the two entries bit for bit.  The warm family: the warm count, warm code 1 and the final mu of ipm_warm(start=...); below the warm count the documented
fallback, the figures of the cold restart at iterate k and iters_total = 2 k.
The last test prints the worst deviation per family and figure (profiles/qp_path_gpu.txt is that output; profiles/qp_path_mutations.txt lists what the
file does to mutated kernels)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import qp_path_reference as qr  # noqa: E402
from qp_path_reference import pq, wr  # noqa: E402
from tunempc_amd import mpc_qp, periodic_qp  # noqa: E402

ENTRIES = ('numpy', 'torch')
FIELDS = ('status', 'iters', 'mu', 'rp', 'rd', 'pivmin')
WORST = {}                                   # (family, figure) -> [largest relative deviation above SPLIT, largest absolute one below, largest excess]


def to_dev(x):
    return x if x is None or isinstance(x, str) else torch.from_numpy(np.array(x, order='C')).cuda()      # (a copy: some case arrays are read-only views)


def scalar(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(-1)[0]


def call_mpc(c, entry, k, **extra):
    """One mpc_qp_batch call of a case (nb = ns = 1) with max_iter = k -> dict of the fields, iters = iters_total, and the whole output under 'out'."""
    pr = c['pr']
    f = to_dev if entry == 'torch' else (lambda x: x)
    extra = {key: ({g: f(v) for g, v in val.items()} if isinstance(val, dict) else val) for key, val in extra.items()}
    out = mpc_qp.mpc_qp_batch(f(pr['A']), f(pr['B']), f(pr['H']), f(pr['X0']), pr['N'], pr['k0'], max_iter=k, **{key: f(v) for key, v in pr['opt'].items()}, **extra)
    return dict(status=int(scalar(out['status'])), iters=int(scalar(out['iters_total'])), mu=float(scalar(out['mu'])), rp=float(scalar(out['rp'])),
                rd=float(scalar(out['rd'])), pivmin=float(scalar(out['pivmin'])), out=out)


def call_periodic(c, entry, k):
    bt = pq.batch_of(c['c'])
    if entry == 'torch':
        bt = {key: (to_dev(v) if hasattr(v, 'shape') else v) for key, v in bt.items()}
    out = periodic_qp.periodic_qp_batch(**bt, max_iter=k)
    return dict(status=int(scalar(out['status'])), iters=int(scalar(out['iters'])), mu=float(scalar(out['mu'])), rp=float(scalar(out['rp'])),
                rd=float(scalar(out['rd'])), pivmin=float(scalar(out['pivmin'])), out=out)


def walk(c, entry, K, **extra):
    """The K calls -> dict of arrays [K + 1] (entry 0 unused: max_iter >= 1)."""
    call = call_periodic if c['fam'] == 'periodic' else call_mpc
    pt = {f: np.full(K + 1, np.nan) for f in FIELDS}
    for k in range(1, K + 1):
        o = call(c, entry, k, **extra)
        for f in FIELDS:
            pt[f][k] = o[f]
    return pt


def note(fam, f, got, ref, cls):
    rel, ab = qr.deviation(got, ref, cls)
    w = WORST.setdefault((fam, f), [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], rel.max()), max(w[1], ab.max()), max(w[2], qr.excess(got, ref, cls).max())


def against_truth(c, pt, truth, n_truth, K, figures=qr.FIGURES):
    """The assertions on one walked path."""
    name, cls = c['fam'] + '/' + c['name'], c['cls']
    conv = np.flatnonzero(pt['status'][1:] == 0)
    n = int(conv[0]) + 1 if len(conv) else None
    print('%s: count %s (reference %d)' % (name, n, n_truth))
    for f in figures:
        print('   %-6s gpu   %s' % (f, ' '.join('%.3e' % x for x in pt[f][1:])))
        print('   %-6s truth %s' % (f, ' '.join('%.3e' % x for x in truth[f][1:K + 1])))
    # the figures first, iterate by iterate: the message names the first k and figure that leave the tolerance
    ex = {f: qr.excess(pt[f][1:], truth[f][1:K + 1], cls) for f in figures}
    if n is not None and (cls == 'plain' or n == n_truth):
        for f in figures:
            note(c['fam'], f, pt[f][1:], truth[f][1:K + 1], cls)
    for k in range(1, K + 1):
        if cls == 'eq' and n is not None and n != n_truth and k >= min(n, n_truth):
            break                                # (a count one apart: from there on one side holds a converged iterate, the other not yet)
        for f in figures:
            assert ex[f][k - 1] <= 1.0, '%s: %s of iterate k = %d is %.6e, reference %.6e: %.1f times the tolerance' % (name, f, k, pt[f][k], truth[f][k], ex[f][k - 1])
    assert (pt['pivmin'][1:] > 0).all() and (np.diff(pt['pivmin'][1:]) <= 0).all(), (name, pt['pivmin'])
    # status and count
    assert n is not None, '%s: no convergence within max_iter = %d (reference %d)' % (name, K, n_truth)
    ks = np.arange(K + 1)
    assert (pt['status'][1:n] == 1).all() and (pt['iters'][1:n] == ks[1:n]).all(), (name, pt['status'], pt['iters'])
    assert (pt['status'][n:] == 0).all() and (pt['iters'][n:] == n).all(), (name, pt['status'], pt['iters'])
    if cls == 'plain':
        assert n == n_truth, '%s: count %d, reference %d' % (name, n, n_truth)
    else:
        assert abs(n - n_truth) <= 1, '%s: count %d, reference %d' % (name, n, n_truth)
        for f in figures:                        # the converged figures of both sides
            assert qr.excess(pt[f][K], truth[f][K], cls) <= 1.0, (name, f, pt[f][K], truth[f][K])


def both_entries(c, K, **extra):
    a, b = (walk(c, e, K, **extra) for e in ENTRIES)
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg='%s/%s: %s differs between the entries' % (c['fam'], c['name'], f))
    return a


@pytest.mark.parametrize('c', qr.mpc_cases(), ids=lambda c: c['fam'] + '-' + c['name'])
def test_mpc_path_against_the_truth_path(c):
    truth, n_truth = qr.mpc_walk(c, 'truth')
    K = len(truth['mu']) - 1
    against_truth(c, both_entries(c, K), truth, n_truth, K)


@pytest.mark.parametrize('c', qr.periodic_cases(), ids=lambda c: c['name'])
def test_periodic_path_and_pivots_against_the_truth_path(c):
    truth, n_truth = qr.periodic_walk(c, 'truth')
    K = len(truth['mu']) - 1
    against_truth(c, both_entries(c, K), truth, n_truth, K, figures=qr.FIGURES + ('pivmin',))


def test_warm_start_count_and_the_fallback_below_it():
    """mpc_qp_batch(guess=...): with max_iter at least the warm count the warm start delivers (code 1) with the count and the final mu of ipm_warm(start=...);
    with max_iter = k below it the warm attempt ends with status 1 and the instance is solved again from the cold start under the same max_iter (the header:
    "a warm-started solve that ends with status 1 or 2 is solved again from the cold start and the iteration counts add up"): the figures are the cold
    path's at iterate k and iters_total = 2 k while k is below the cold count too."""
    c = qr.warm_case()
    warm, n_warm = qr.mpc_walk(c, 'truth')
    cold_case = dict(c, fam='hard', start=None)
    cold, n_cold = qr.mpc_walk(cold_case, 'truth')
    K = max(n_warm, n_cold) + 1
    if K > len(cold['mu']) - 1:
        cold, _ = qr.mpc_walk(cold_case, 'truth', K=K)
    if K > len(warm['mu']) - 1:
        warm, _ = qr.mpc_walk(c, 'truth', K=K)
    g = c['guess']
    guess = dict(X=g['X'][None, None], U=g['U'][None, None], lam=g['Lam'][None, None])
    print('warm count %d, cold count %d' % (n_warm, n_cold))
    assert n_warm < n_cold                                                   # (the case: a good guess)
    seen = {}
    for e in ENTRIES:
        rows = []
        for k in range(1, K + 1):
            o = call_mpc(c, e, k, guess=guess)
            code = int(scalar(o['out']['warm']))
            rows.append([o[f] for f in FIELDS] + [code])
            print('   %s max_iter %d: status %d iters_total %d warm %d mu %.3e rp %.3e rd %.3e' % (e, k, o['status'], o['iters'], code, o['mu'], o['rp'], o['rd']))
            if k >= n_warm:
                assert o['status'] == 0 and o['iters'] == n_warm and code == wr.WARM, (k, o['status'], o['iters'], code)
                ref = warm
            else:
                assert k < n_cold and o['status'] == 1 and o['iters'] == 2 * k and code == wr.FAILED, (k, o['status'], o['iters'], code)
                ref = cold
                alone = call_mpc(cold_case, e, k)                            # the cold call itself: the same bits
                assert all(alone[f] == o[f] for f in ('mu', 'rp', 'rd')), (k, alone, o)
            for f in qr.FIGURES:
                note('warm', f, np.array([o[f]]), ref[f][k:k + 1], 'plain')
                ex = qr.excess(o[f], ref[f][k], 'plain')
                assert ex <= 1.0, 'warm, max_iter %d: %s is %.6e, reference %.6e: %.1f times the tolerance' % (k, f, o[f], ref[f][k], ex)
        seen[e] = rows
    assert seen['numpy'] == seen['torch']


def test_zz_report_the_worst_deviations():
    """Prints what the tests above measured: per family and figure the largest relative deviation (reference above SPLIT), the largest absolute one (below)
    and the largest fraction of the tolerance that was used."""
    print('\nfamily   figure   relative   absolute   of the tolerance')
    for (fam, f), w in sorted(WORST.items()):
        print('%-8s %-6s   %8.1e   %8.1e   %6.3f' % (fam, f, w[0], w[1], w[2]))
    assert WORST and all(w[2] <= 1.0 for w in WORST.values())
