"""The reference side of the interior-point PATH tests (tests/qp_path_reference.py; no GPU): every path case is walked by two independent means (three in the
periodic family), the largest spread between them per class and figure is measured and held against the class tolerances that test_gpu_qp_path.py uses, the
conditions on the cases are checked, three mutations of the references are shown to leave the tolerance within three iterates, and the stall of the staged
restatement of the periodic Newton step is pinned to its cause.

`python tests/test_qp_path_cpu.py` prints the spread table (profiles/qp_path_spread.txt is that output)."""
import functools

import numpy as np
import pytest

import qp_path_reference as qr
from qp_path_reference import pq

ALL_FIGURES = qr.FIGURES + ('pivmin',)
FAMILIES = ('hard', 'soft', 'eq', 'affine', 'quad', 'warm', 'periodic')


def all_cases():
    return qr.mpc_cases() + [qr.warm_case()] + qr.periodic_cases()


def paths_of(c):
    return qr.periodic_paths(c) if c['fam'] == 'periodic' else qr.mpc_paths(c)


@functools.lru_cache(maxsize=None)
def spreads():
    """-> ({(class, figure): [largest relative spread, largest absolute spread]}, the lines of the table).  The means: the reference as it is and, in the
    periodic family, the staged elimination of the kernel, each against the truth path; iterates 1 .. K (iterate 0 is the start: no linear algebra yet)."""
    worst = {(cls, f): [0.0, 0.0] for cls in ('plain', 'eq') for f in ALL_FIGURES}
    lines = ['%-8s %-22s %-5s %2s  %s' % ('family', 'case', 'class', 'n', '  '.join('%-19s' % (f + ' rel / abs') for f in ALL_FIGURES))]
    for c in all_cases():
        ps = paths_of(c)
        cell = []
        for f in ALL_FIGURES:
            if np.isnan(ps['truth'][f]).all():
                cell.append('%-19s' % '-')
                continue
            rel = ab = 0.0
            for means in ('plain', 'staged'):
                if means in ps:
                    r, a = qr.deviation(ps[means][f][1:], ps['truth'][f][1:], c['cls'])
                    rel, ab = max(rel, r.max()), max(ab, a.max())
            w = worst[(c['cls'], f)]
            w[0], w[1] = max(w[0], rel), max(w[1], ab)
            cell.append('%8.1e / %8.1e' % (rel, ab))
        lines.append('%-8s %-22s %-5s %2d  %s' % (c['fam'], c['name'], c['cls'], ps['n_truth'], '  '.join(cell)))
    lines.append('')
    for cls in ('plain', 'eq'):
        for f in ALL_FIGURES:
            lines.append('largest spread, class %-5s %-6s: relative %8.1e  absolute %8.1e' % (cls, f, *worst[(cls, f)]))
        rel, ab = (max(worst[(cls, f)][i] for f in ALL_FIGURES) for i in (0, 1))
        lines.append('class %-5s: figures above SPLIT = %g relative, below absolute; 100 x the largest spread = %.1e / %.1e; REL = %g, ABS = %g'
                     % (cls, qr.SPLIT[cls], qr.MARGIN * rel, qr.MARGIN * ab, qr.REL[cls], qr.ABS[cls]))
    return worst, lines


def test_the_spread_of_the_means_stays_100_times_inside_the_class_tolerances():
    worst, lines = spreads()
    print('\n'.join(lines))
    for cls in ('plain', 'eq'):
        rel, ab = (max(worst[(cls, f)][i] for f in ALL_FIGURES) for i in (0, 1))
        assert qr.MARGIN * rel <= qr.REL[cls] and qr.MARGIN * ab <= qr.ABS[cls], (cls, rel, ab)
        # ... and the constants are that figure rounded up, not something wider (a factor 3 for another BLAS or another libm)
        assert qr.REL[cls] <= 3 * qr.round_up(qr.MARGIN * rel) and qr.ABS[cls] <= 3 * qr.round_up(qr.MARGIN * ab), (cls, rel, ab)


@pytest.mark.parametrize('c', all_cases(), ids=lambda c: c['fam'] + '-' + c['name'])
def test_every_case_converges_with_its_certificate_on_both_paths(c):
    ps = paths_of(c)
    assert ps['n_plain'] is not None and ps['n_truth'] is not None
    if c['fam'] == 'periodic':
        r = pq.solve_case(c['c'])
        assert r['a']['status'] == 0 and r['b']['certificate'] and r['b']['nact'] >= 1, c['name']
        assert ps['n_staged'] is not None and abs(ps['n_staged'] - ps['n_truth']) <= (0 if c['cls'] == 'plain' else 1)
    else:
        status, cert, nact = qr.mpc_certificate(c)
        assert status == 0 and cert and nact >= 1, (c['name'], status, cert, nact)
    if c['cls'] == 'plain':
        # the count is no coin toss: the deciding figure of the stop test is a factor 2 away from its threshold at the last two iterates
        n = ps['n_truth']
        assert ps['n_plain'] == n
        r0, r1 = qr.stop_ratio(ps['truth'], n - 1), qr.stop_ratio(ps['truth'], n)
        print(c['name'], 'stop test at n - 1, n: %.2e %.2e of the threshold' % (r0, r1))
        assert r0 >= 2.0 and r1 <= 0.5, (c['name'], r0, r1)
    else:
        assert abs(ps['n_plain'] - ps['n_truth']) <= 1
    # status and count along the path: 1 with iters = k before convergence, 0 with a constant count from then on
    pt, n = ps['truth'], ps['n_truth']
    assert (pt['status'][:n] == 1).all() and (pt['iters'][:n] == np.arange(n)).all() and (pt['status'][n:] == 0).all() and (pt['iters'][n:] == n).all()


def relative_iterates(c):
    """The iterates k >= 1 of the truth path where mu, rp and rd all exceed 1e3 ABS of the class."""
    pt = paths_of(c)['truth']
    return [k for k in range(1, len(pt['mu'])) if min(pt[f][k] for f in qr.FIGURES) > 1e3 * qr.ABS[c['cls']]]


@pytest.mark.parametrize('fam', [f for f in FAMILIES if f != 'warm'])      # (a warm start lies next to the solution: its path is short)
def test_every_family_has_a_case_that_is_compared_relatively_at_three_iterates(fam):
    """In the class 'plain' this holds in every family.  The family 'eq' has only cases of the class 'eq', and there it CANNOT hold: the noise of the weight
    1 / RHO in r_d is absolute (1e-4 of the equality residual of the step before: 5.4e-6 on the path cases here, 5e-5 on periodic case_odd), so
    1e3 ABS['eq'] = 0.6 is above mu, rp or rd at every iterate but the start.  That family is compared mostly absolutely; its counts are printed, and the
    mutations below are still seen on every one of its cases within three iterates."""
    counts = {c['name']: len(relative_iterates(c)) for c in all_cases() if c['fam'] == fam}
    print(fam, counts)
    if fam == 'eq':
        assert max(counts.values()) < 3          # (if this ever fails the condition can be asserted for this family too)
    else:
        assert max(counts.values()) >= 3, counts


@pytest.mark.parametrize('which', qr.MUTATIONS)
@pytest.mark.parametrize('c', all_cases(), ids=lambda c: c['fam'] + '-' + c['name'])
def test_a_mutated_reference_leaves_the_tolerance_within_three_iterates(c, which):
    truth = paths_of(c)['truth']
    K = 3
    mut = qr.periodic_mutant_walk(c, which, K) if c['fam'] == 'periodic' else qr.mpc_mutant_walk(c, which, K)
    ex = {f: qr.excess(mut[f][:K + 1], truth[f][:K + 1], c['cls']) for f in qr.FIGURES}
    first = [(k, f, ex[f][k]) for k in range(K + 1) for f in qr.FIGURES if ex[f][k] > 1.0]
    print(c['fam'], c['name'], which, 'first beyond the tolerance:', first[:1])
    assert first, {f: ex[f].tolist() for f in ex}
    assert all(ex[f][0] == 0.0 for f in qr.FIGURES)                          # the start is the same


@pytest.mark.parametrize('c', qr.stall_cases(), ids=lambda c: c['name'])
def test_the_stall_of_the_staged_restatement_is_a_defect_of_its_composition(c):
    """The Newton step of csrc/tmpc_periodic_qp.h restated in numpy (newton_border) and composed into the iteration stalled at r_d ~ 1e-4 .. 1e-5 on the cases
    with equality rows where the dense paths converge.  Cause: the composition took dlam, ds, dnu from the sweep's dv by the kernel's formulas but with the
    row residuals G v + s - h and Je v - re EVALUATED AGAIN on the dense problem.  They differ from the residuals inside the right-hand side by one rounding,
    and dlam = w (..), dnu = (1 / RHO)(J dz + r_eq) multiply that by up to 1 / RHO = 1e12: a noise of 1e-4 in the multipliers that does not shrink with the
    step, so no later step removes it.  It is no property of the staged elimination at the weight 1 / RHO and nothing rescues the kernel: it keeps r_in and
    r_eq of pass 1 (RIN, REQ) and its forward sweep reads them back.  With the same residuals reused (newton_staged(reuse=True)) the restatement converges
    like the dense paths."""
    ps = qr.periodic_paths(c)
    K = ps['K']
    bad, n_bad = qr.periodic_walk(c, 'recomputed', K=K)
    good, truth = ps['staged'], ps['truth']
    print(c['name'], 'count: truth %s, staged %s, staged with recomputed residuals %s' % (ps['n_truth'], ps['n_staged'], n_bad))
    print('   rd truth      ', ' '.join('%.1e' % x for x in truth['rd']))
    print('   rd staged     ', ' '.join('%.1e' % x for x in good['rd']))
    print('   rd recomputed ', ' '.join('%.1e' % x for x in bad['rd']))
    assert ps['n_staged'] is not None and abs(ps['n_staged'] - ps['n_truth']) <= 1
    # the recomputed composition is stuck above tol at an iterate where the reused one has converged; mu and rp are not affected
    assert bad['rd'][K] > 1e3 * good['rd'][K] and bad['rd'][K] > qr.mq.TOL and good['rd'][K] <= qr.mq.TOL
    assert bad['rp'][K] <= qr.mq.TOL and good['rp'][K] <= qr.mq.TOL


if __name__ == '__main__':
    print('Spread of the interior-point path between independent means on the CPU (tests/test_qp_path_cpu.py; iterates 1 .. n + 1 of every path case).')
    print('Means: the reference as it is (fp64 LU; Je\' Je / RHO in the matrix) and, periodic family, the staged elimination of the kernel, each against the')
    print('truth path (LU refined with longdouble residuals; class eq: the augmented system).\n')
    print('\n'.join(spreads()[1]))
