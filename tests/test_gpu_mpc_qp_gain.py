"""GPU tests of the local gain of a solved MPC step (csrc/tmpc_mpc_qp_gain.h, tunempc_amd.mpc_qp.mpc_qp_gain_batch and the certificate
mpc_gain_equivalence_batch) against tests/mpc_qp_gain_reference.py, on solutions that mpc_qp_batch returned on the GPU.

Bounds.  K0, Pi0 against method (a) of the reference, run at the GPU's own solution: PARITY = 1e-8 relative to max(1, max|.|), the bound
tests/test_gpu_horizon_lqr.py holds the same stage to; cnt0, cntall and cls are equal exactly.  Two GPU paths of one stage (all rows free against
horizon_lqr_batch, the expanded emulation through horizon_lqr_batch): ten times the disagreement of the reference's methods (a) and (c) on the same instance
(with every row free: of the case), as test_mpc_qp_gain_cpu.py measures and mpc_qp_gain_reference.KKT_MEASURED stores it, floor 1e-13.  Open-loop sensitivities: dX d, dU d against the increment of the polished reference solution from x_0 to x_0 + d, divided by max|d|, to the
(a)-against-(b) bound of the case (ten times what test_mpc_qp_gain_cpu.py measures).  Certificate: dK0_rel within PARITY, du0 within the 2e-8 that
tests/test_gpu_mpc_qp.py holds u0 to."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_soft_reference as ms  # noqa: E402
import mpc_qp_eq_reference as eqr  # noqa: E402
import mpc_qp_quad_reference as mqq  # noqa: E402
import mpc_qp_gain_reference as gr  # noqa: E402

PARITY = 1e-8
U0_BOUND = 2e-8
ENTRIES = ['host', 'device']
ROWS = ('D', 'd', 'ndcnt', 'Pf', 'penalty', 'penalty2', 'J', 'necnt', 'terminal')


def to_dev(x):
    return None if x is None else torch.from_numpy(np.array(x, order='C')).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def mover(entry):
    return (lambda x: to_dev(x) if isinstance(x, np.ndarray) else x) if entry == 'device' else (lambda x: x)


def solve(entry, bt):
    """mpc_qp_batch on a batch dict (the keys of mpc_qp_eq_reference.batch_of, optionally penalty2) -> the dict as the entry returned it."""
    from tunempc_amd import mpc_qp as m
    f = mover(entry)
    kw = {k: f(bt[k]) for k in ROWS + ('q', 'r') if bt.get(k) is not None}
    return m.mpc_qp_batch(f(bt['A']), f(bt['B']), f(bt['H']), f(bt['X0']), bt['N'], bt['k0'], **kw)


def gain(entry, bt, sol, **kw):
    from tunempc_amd import mpc_qp as m
    f = mover(entry)
    rows = {k: f(bt[k]) for k in ROWS if bt.get(k) is not None}
    rows.update({k: f(v) for k, v in kw.items()})
    return m.mpc_qp_gain_batch(f(bt['A']), f(bt['B']), f(bt['H']), sol, bt['N'], bt['k0'], **rows)


def check_parity(bt, sol, g, label, cls=None):
    """The outputs g of mpc_qp_gain_batch (numpy, return_all) against method (a) at the solutions sol (numpy) -> the worst relative difference."""
    ref = gr.reference_of_batch(bt, sol, cls)
    worst = 0.0
    for b, row in enumerate(ref):
        for s, (r, c, strict) in enumerate(row):
            assert not r['infeasible'] and g['status'][b, s] == 0, (label, b, s, g['status'][b, s])
            np.testing.assert_array_equal(g['cls'][b, s], c, err_msg='%s cls[%d, %d]' % (label, b, s))
            assert g['cnt0'][b, s] == r['cnt'][0] and np.array_equal(g['cntall'][b, s], r['cnt']), (label, b, s, g['cntall'][b, s], r['cnt'])
            assert np.array_equal(g['nactive'][b, s], (c > 0).sum(axis=1))
            ek, ep, ea = gr.rel(g['K0'][b, s], r['K0']), gr.rel(g['Pi0'][b, s], r['Pi0']), gr.rel(g['Kall'][b, s], r['K'])
            PzG = np.eye(r['Pz0'].shape[0]) - g['Hn0'][b, s].T @ g['Hn0'][b, s]
            print('%s[%d, %d]: active per stage %s, cnt %s, strict %.6f (reference %.6f), K0 %.2e, Pi0 %.2e, Kall %.2e, feas %.1e' % (
                label, b, s, g['nactive'][b, s].tolist(), g['cntall'][b, s].tolist(), g['strict'][b, s], strict, ek, ep, ea, g['feas'][b, s]))
            assert abs(g['strict'][b, s] - strict) <= 1e-6 and g['feas'][b, s] <= 1e-9
            assert np.abs(PzG - r['Pz0']).max() <= PARITY
            worst = max(worst, ek, ep, ea)
    assert worst <= PARITY, (label, worst)
    return worst


# ----------------------------------------------------------------------------- 1. parity on hard rows
def case_mixed_small_N2():
    return mq.case_mixed_small(2)


HARD = [mq.case_box_nu1, mq.case_box_nu2, mq.case_mixed_small, case_mixed_small_N2, mq.case_single_phase, mq.case_box_bench, gr.case_state_box]


@pytest.mark.parametrize('case', HARD, ids=lambda c: c.__name__)
def test_parity_with_the_reference_at_the_solutions_of_the_gpu(case):
    """p 3 / nx 3 / nu 1 at N 5 from phase 2 (the phase wraps), p 3 / nx 3 / nu 2 at N 4 and N 2 < p (ragged ndcnt, instances with different active counts, stages
    without an active row), p 1, the bench stage shape (the layout) and the state box (active state rows, two active rows at a stage of two inputs)."""
    bt = gr.batch_of_case(case())
    sol = solve('device', bt)
    assert int(sol['status'].max()) == 0
    g = to_host(gain('device', bt, sol, return_all=True))
    check_parity(bt, to_host(sol), g, case.__name__)
    assert g['strict'].min() >= 0.99
    if case in (mq.case_mixed_small, gr.case_state_box):                     # what the docstring says of them
        total = g['nactive'][0].sum(axis=1)
        assert len(set(total.tolist())) > 1, total                           # instances of one problem with different active counts in one launch
        assert ((g['nactive'][0] == 0).any(axis=1) & (total > 0)).any()      # a stage without an active row in an instance that has active rows


# ----------------------------------------------------------------------------- 2. the same stage on two GPU paths
def test_all_rows_free_is_the_horizon_pass():
    from tunempc_amd import lqr
    for case in (mq.case_box_nu2, gr.case_state_box, mq.case_box_bench):
        bt = gr.batch_of_case(case())
        sol = solve('device', bt)
        nb, ns = bt['X0'].shape[:2]
        g = to_host(gain('device', bt, sol, active=np.zeros((nb, ns, bt['N'], bt['D'].shape[2]), np.int32)))
        h = to_host(lqr.horizon_lqr_batch(to_dev(bt['A']), to_dev(bt['B']), to_dev(bt['H']), bt['N'], terminal='cost', Pf=to_dev(bt['Pf']), phases=[bt['k0']]))
        bound = gr.two_paths_bound(case)                                     # every row free: one stored figure per case
        for s in range(ns):
            ek, ep = gr.rel(g['K0'][0, s], h['K0'][0, 0]), gr.rel(g['Pi0'][0, s], h['Pi0'][0, 0])
            print('%s[%d]: all rows free against horizon_lqr_batch: K0 %.2e, Pi0 %.2e (bound %.1e)' % (case.__name__, s, ek, ep, bound))
            assert ek <= bound and ep <= bound and g['cnt0'][0, s] == 0 and not g['cls'][0, s].any()


def test_expanded_emulation_through_the_horizon_entry_on_the_state_box():
    """One "problem" per instance with p = N, the class-1 rows gathered on the host as J: what the gain pass replaces."""
    from tunempc_amd import lqr
    c = gr.case_state_box()
    bt = gr.batch_of_case(c)
    sol = solve('device', bt)
    g = to_host(gain('device', bt, sol))
    ns, N = bt['X0'].shape[1], bt['N']
    Es = [gr.expand(bt['A'][0], bt['B'][0], bt['H'][0], N, bt['k0'], g['cls'][0, s], bt['D'][0], None, bt['Pf'][0]) for s in range(ns)]
    nr = max(1, max(0 if E['J'] is None else E['J'].shape[1] for E in Es))
    n = bt['H'].shape[2]
    J = np.zeros((ns, N, nr, n))
    for s, E in enumerate(Es):
        if E['J'] is not None:
            J[s, :, :E['J'].shape[1]] = E['J']
    st = lambda k: to_dev(np.stack([E[k] for E in Es]))
    h = to_host(lqr.horizon_lqr_batch(st('A'), st('B'), st('H'), N, terminal='cost', Pf=st('Pf'), phases=[0], J=to_dev(J),
                                      ncnt=to_dev(np.stack([E['rows'] for E in Es]).astype(np.int32))))
    for s in range(ns):
        bound = gr.two_paths_bound(gr.case_state_box, s)                     # the stored figure of the same instance
        ek, ep = gr.rel(g['K0'][0, s], h['K0'][s, 0]), gr.rel(g['Pi0'][0, s], h['Pi0'][s, 0])
        print('state box[%d]: against the emulation: K0 %.2e, Pi0 %.2e (bound %.1e), cnt0 %d / %d' % (s, ek, ep, bound, g['cnt0'][0, s], h['cnt0'][s, 0]))
        assert ek <= bound and ep <= bound and g['cnt0'][0, s] == h['cnt0'][s, 0] and h['status'][s, 0] == 0


# ----------------------------------------------------------------------------- 3. the scalar case
def test_an_active_input_bound_at_stage_0_of_one_input_gives_a_zero_gain():
    from tunempc_amd import lqr
    bt = gr.batch_of_case(mq.case_box_nu1())
    sol = solve('device', bt)
    g = to_host(gain('device', bt, sol))
    h = to_host(lqr.horizon_lqr_batch(to_dev(bt['A']), to_dev(bt['B']), to_dev(bt['H']), bt['N'], terminal='cost', Pf=to_dev(bt['Pf']), phases=[bt['k0']]))
    act0 = g['nactive'][0, :, 0]
    assert (act0 == 1).any() and (g['nactive'][0].sum(axis=1) == 0).any()
    for s in range(bt['X0'].shape[1]):
        if act0[s] == 1:
            assert np.abs(g['K0'][0, s]).max() <= 1e-13, g['K0'][0, s]
        elif g['nactive'][0, s].sum() == 0:
            assert gr.rel(g['K0'][0, s], h['K0'][0, 0]) <= gr.KKT_FLOOR


# ----------------------------------------------------------------------------- 4. open-loop sensitivities
@pytest.mark.parametrize('case', [mq.case_mixed_small, gr.case_state_box], ids=lambda c: c.__name__)
def test_open_loop_sensitivities_reproduce_the_polished_solution_nearby(case):
    bt = gr.batch_of_case(case())
    g = to_host(gain('device', bt, solve('device', bt), return_all=True))
    insts = gr.hard_instances(case)
    rng = np.random.default_rng(3)
    worst = 0.0
    for s, (i, r) in enumerate(zip(insts, gr.solved(case.__name__, insts))):
        Pz = np.eye(i['A'].shape[1]) - g['Hn0'][0, s].T @ g['Hn0'][0, s]
        dx = 1e-3 * Pz @ rng.standard_normal(i['A'].shape[1])
        P = mq.dense(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'] + dx, **i['kw'])
        b = mqq.polish_quad(P, r['cvec'], r['zvec'], r['state'])
        assert b['certificate'] and np.array_equal(b['state'], r['state'])      # the active set is unchanged at x_0 + dx
        X, U, _ = mq.unpack(P, b['v'])
        sc = np.abs(dx).max()
        ex = np.abs(g['dX'][0, s] @ dx - (X - r['X'])).max() / sc / max(1.0, np.abs(g['dX'][0, s]).max())
        eu = np.abs(g['dU'][0, s] @ dx - (U - r['U'])).max() / sc / max(1.0, np.abs(g['dU'][0, s]).max())
        print('%s[%d]: dX %.2e, dU %.2e (bound %.1e)' % (case.__name__, s, ex, eu, gr.ab_bound(case)))
        assert np.array_equal(g['dU'][0, s, 0], -g['K0'][0, s]) or gr.rel(g['dU'][0, s, 0], -g['K0'][0, s]) <= 1e-15
        worst = max(worst, ex, eu)
    assert worst <= gr.ab_bound(case)


# ----------------------------------------------------------------------------- 5. row kinds
def test_soft_rows_violated_and_active():
    """L1 rows: a violated row drops out (class 0), an active one is an equality (class 1); with the weight far above the multipliers the hard classes."""
    i = ms.infeasible_instance()
    bt = dict(ms.batch_of([i]), J=None, r=None, necnt=None, terminal=None)
    sol = solve('device', bt)
    assert int(sol['status'].max()) == 0 and int(sol['nviol'].max()) >= 0
    g = to_host(gain('device', bt, sol, return_all=True))
    check_parity(bt, to_host(sol), g, 'soft violated')
    h = to_host(sol)
    viol = h['eps'][0, 0] > 1e-3
    assert viol.any() and not g['cls'][0, 0][viol].any() and (g['cls'][0, 0] == 1).any() and not (g['cls'] == 2).any()
    insts = ms.instances(mq.case_box_nu2, 1e3)
    bt = dict(ms.batch_of(insts), J=None, r=None, necnt=None, terminal=None)
    sol = solve('device', bt)
    g = to_host(gain('device', bt, sol, return_all=True))
    check_parity(bt, to_host(sol), g, 'soft active')
    hard = gr.batch_of_case(mq.case_box_nu2())
    gh = to_host(gain('device', hard, solve('device', hard)))
    assert np.array_equal(g['cls'][:, 0], gh['cls'][0]) and (g['cls'] == 1).any()
    assert gr.rel(g['K0'][:, 0], gh['K0'][0]) <= PARITY


def test_pure_quadratic_and_l1_l2_rows():
    for label, (c, Z) in (('pure quadratic', (0.0, 500.0)), ('L1 + L2', (50.0, 500.0))):
        i = mqq.infeasible_instance(c, Z)
        i2 = dict(i, x0=0.05 * i['x0'] / np.abs(i['x0']).max())              # inside the bound: every row inactive
        bt = dict(mqq.batch_of([i, i2]), J=None, r=None, necnt=None, terminal=None)
        sol = solve('device', bt)
        assert int(sol['status'].max()) == 0
        g = to_host(gain('device', bt, sol, return_all=True))
        check_parity(bt, to_host(sol), g, label)
        assert (g['cls'][0] == 2).any() and not g['cls'][1].any(), g['cls']


@pytest.mark.parametrize('case', [eqr.case_term_box_nu2, eqr.case_tx_box_nu2, eqr.case_rows_mixed_small, eqr.case_rows_mixed_small_N2, eqr.case_term_p1],
                         ids=lambda c: c.__name__)
def test_equality_rows_and_terminal_rows(case):
    """terminal='constraint', a Tx with nt = 2 < nx = 3, ragged J rows with terminal rows (N = 4 and N = 2 < p), p = 1."""
    bt = eqr.batch_of(case())
    sol = solve('device', bt)
    assert int(sol['status'].max()) == 0
    g = to_host(gain('device', bt, sol, return_all=True))
    check_parity(bt, to_host(sol), g, case.__name__)
    if isinstance(bt['terminal'], str):
        assert g['cntall'].max() >= 1                                        # x_N = 0 reaches back into the horizon as a constraint-to-go
    free = to_host(gain('device', dict(bt, terminal=None), sol, return_all=True))
    assert np.abs(free['Kall'] - g['Kall']).max() > 1e-3                     # the terminal rows are seen by the pass


# ----------------------------------------------------------------------------- 6. the certificate
def _certificate(bt, H, P, entry):
    from tunempc_amd import mpc_qp as m
    f = mover(entry)
    kw = {k: f(bt[k]) for k in ('D', 'd', 'ndcnt', 'q', 'Pf') if bt.get(k) is not None}
    return m.mpc_gain_equivalence_batch(f(bt['A']), f(bt['B']), f(H), f(bt['H']), f(bt['X0']), bt['N'], P=f(P), phase0=bt['k0'], **kw)


@pytest.mark.parametrize('entry', ENTRIES)
def test_certificate_on_the_state_box_and_on_mixed_small(entry):
    """Both sides of lqr_horizon_reference.case_ragged_rows (Hc: the tracking side of the two cases, H and P: its economic side)."""
    import lqr_horizon_reference as lh
    base = lh.case_ragged_rows()
    for name, bt in (('state box', gr.batch_of_case(gr.case_state_box())), ('mixed small', gr.batch_of_case(mq.case_mixed_small()))):
        assert np.array_equal(bt['H'], base['Hc'])
        o = _certificate(bt, base['H'], base['P'], entry)
        print('%s (%s): dK0_rel %s, du0 %s, same_active %s, strict %s, statuses %s %s %s %s' % (
            name, entry, o['dK0_rel'].ravel(), o['du0'].ravel(), o['same_active'].ravel(), o['strict'].ravel(), o['status_qp_H'].ravel(), o['status_qp_Hc'].ravel(),
            o['status_H'].ravel(), o['status_Hc'].ravel()))
        assert not o['status_qp_Hc'].any() and not o['status_Hc'].any() and not o['status_H'].any() and not o['status_qp_H'].any()
        assert o['same_active'].all() and o['dK0_rel'].max() <= PARITY and o['du0'].max() <= U0_BOUND and o['subspace_diff'].max() <= PARITY
        assert o['strict'].min() >= 0.99


def test_certificate_with_an_instance_that_fails_on_the_tracking_side():
    """x_0 outside the hard state box: a row of stage 0 on x_0 alone that x_0 violates, status 1 of the solve and a NaN solution.  That instance returns NaN /
    False with its statuses; its neighbours return the bits of the batch without it."""
    import lqr_horizon_reference as lh
    base = lh.case_ragged_rows()
    bt = gr.batch_of_case(gr.case_state_box())
    clean = _certificate(bt, base['H'], base['P'], 'device')
    X0 = bt['X0'].copy(); X0[0, 1, 0] = 5.0
    for entry in ENTRIES:
        o = _certificate(dict(bt, X0=X0), base['H'], base['P'], entry)
        assert o['status_qp_Hc'][0].tolist() == [0, 1, 0, 0] and o['status_Hc'][0].tolist() == [0, 3, 0, 0] and o['status_H'][0, 1] == 3
        assert np.isnan(o['dK0'][0, 1]) and np.isnan(o['dK0_rel'][0, 1]) and np.isnan(o['du0'][0, 1]) and not o['same_active'][0, 1]
        for k in ('du0', 'dK0', 'dK0_rel', 'subspace_diff', 'strict', 'same_active', 'status_qp_H', 'status_qp_Hc', 'status_H', 'status_Hc'):
            np.testing.assert_array_equal(o[k][0, [0, 2, 3]], clean[k][0, [0, 2, 3]], err_msg=k)
        K0 = o['K0'].cpu().numpy() if entry == 'device' else o['K0']
        np.testing.assert_array_equal(K0[0, [0, 2, 3]], clean['K0'].cpu().numpy()[0, [0, 2, 3]])
