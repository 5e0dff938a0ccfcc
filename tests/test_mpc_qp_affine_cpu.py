"""CPU tests of the affine MPC step (dynamics offsets, a linear terminal cost, a terminal right-hand side) and of the loop on a disturbed plant: the conditions
of the cases of tests/mpc_qp_affine_reference.py, its numpy iteration (a) against its truth (b) (the figure that bounds the GPU tests), the shifted cases
against their deviation problems, the case without rows against a condensed dense solve, the loops, about_reference, and what tunempc_amd.mpc_qp and the
library refuse before a device is touched.  No device is needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mpc_qp_eq_reference as eq
import mpc_qp_affine_reference as af

ITERS_MAX = 25                      # measured: 6 .. 12


@pytest.mark.parametrize('case', af.VALUE_CASES, ids=[c.__name__ for c in af.VALUE_CASES])
def test_the_cases_are_well_posed_and_the_iteration_agrees_with_the_polished_solution(case):
    """Every instance: feasible ((a) converges), a valid certificate, margin >= MARGIN_MIN; every case with inequality rows: an active one.  (a) against (b),
    measured (worst figure of the case): shift_term_box_nu1 5.3e-12, shift_tx_box_nu2 8.3e-11, shift_rows_mixed_small 7.3e-13, shift_rows_mixed_small_N2 6.3e-14,
    shift_term_p1 5.3e-13, shift_term_box_bench 2.0e-10, shift_soft 1.5e-13, aff_term_box_nu2 8.9e-11, aff_term_mixed_small 8.7e-12, aff_qf_box_nu1 1.4e-10,
    aff_tx_soft_box_nu2 3.3e-11, aff_bench 1.9e-12, aff_edge 1.0e-14.  The worst, 2.0e-10 (1.97e-10), rounded up: AFF_IPM_VS_POLISH."""
    c = case()
    active = 0
    worst = {}
    for b, rb in enumerate(af.solve_case(c)):
        for s, r in enumerate(rb):
            d = eq.ab_disagreement(r)
            print('   %s instance %d.%d: iters %d margin %.1e nact %d nviol %d | (a) vs (b) %s' % (c['name'], b, s, r['a']['iters'], r['b']['margin'], r['b']['nact'],
                                                                                              r['b']['nviol'], {k: '%.1e' % v for k, v in d.items()}))
            assert r['a']['status'] == 0 and r['a']['iters'] <= ITERS_MAX
            assert r['b']['certificate'] and r['b']['rank_ok'] and r['b']['margin'] >= af.MARGIN_MIN, (r['b']['margin'], r['b']['stat'])
            k = af.kkt_check_aff(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], r['X'], r['U'], r['Lam'], r['Nu'], r['NuT'], r['Eps'],
                                 None if c['penalty'] is None else c['penalty'][b], **af.kwargs(c, b))
            assert max(k['dyn'], k['eq'], k['term'], k['comp'], k['comp_e'], k['stat']) <= 1e-11 and k['viol'] <= 1e-11, k
            active += r['b']['nact']
            for q, v in d.items():
                worst[q] = max(worst.get(q, 0.0), v)
    print('   %s worst %s' % (c['name'], {k: '%.1e' % v for k, v in worst.items()}))
    assert c['D'] is None or active >= 1
    assert max(worst.values()) <= af.AFF_IPM_VS_POLISH, worst


@pytest.mark.parametrize('case', af.AFFINE_CASES, ids=[c.__name__ for c in af.AFFINE_CASES])
def test_the_affine_terms_are_not_small(case):
    """The kkt figures of the solution WITHOUT c, t, qf in the check are far from rounding: the cases exercise what they are named for."""
    c = case()
    r = af.solve_case(c)[0][0]
    kw = dict(af.kwargs(c), offset=None, qf=None, trhs=None)
    k = af.kkt_check_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], r['X'], r['U'], r['Lam'], r['Nu'], r['NuT'], r['Eps'],
                         None if c['penalty'] is None else c['penalty'][0], **kw)
    print('   %s without the affine terms: dyn %.1e term %.1e stat %.1e' % (c['name'], k['dyn'], k['term'], k['stat']))
    assert (c['offset'] is None or k['dyn'] > 1e-3) and (c['trhs'] is None or k['term'] > 1e-3) and (c['qf'] is None or k['stat'] > 1e-3)


@pytest.mark.parametrize('case', af.SHIFT_CASES, ids=[c.__name__ for c in af.SHIFT_CASES])
def test_a_shifted_case_is_its_deviation_problem_plus_the_reference(case):
    """(b) of the absolute problem against (b) of the deviation problem plus the reference, the multipliers against the same multipliers.  Measured (worst
    instance): term_box_nu1 2.1e-15, tx_box_nu2 2.0e-15, rows_mixed_small 4.8e-15, rows_mixed_small_N2 8.8e-15, term_p1 2.5e-15, term_box_bench 5.0e-14
    (4.97e-14), soft 4.6e-15; rounded up: AFF_SHIFT_VS_DEV."""
    c = case()
    assert np.abs(c['offset']).max() > 0.1 and np.abs(c['xref']).max() > 0.5
    worst = 0.0
    for b, (rb, db) in enumerate(zip(af.solve_case(c), eq.solve_case(c['dev']))):
        for s, (r, rd) in enumerate(zip(rb, db)):
            Xs, Us = af.shifted_solution(c, rd, b)
            ls = eq.mult_scale(rd)
            e = max([np.abs(r['X'] - Xs).max() / max(1.0, np.abs(Xs).max()), np.abs(r['U'] - Us).max() / max(1.0, np.abs(Us).max())] +
                    [np.abs(r[k] - rd[k]).max() / ls for k in ('Lam', 'Nu', 'NuT', 'Eps') if r[k].size])
            print('   %s instance %d.%d: %.1e, iters %d (deviation problem %d)' % (c['name'], b, s, e, r['a']['iters'], rd['a']['iters']))
            assert r['nact0'] == rd['nact0'] and r['nviol0'] == rd['nviol0']
            worst = max(worst, e)
    assert worst <= af.AFF_SHIFT_VS_DEV


def test_without_rows_the_step_is_the_affine_lq_problem():
    """(b) without D and J against the condensed dense solve.  Measured: 2.2e-16, 3.4e-16, 6.9e-16 (6.94e-16), 5.6e-16; rounded up: AFF_POLISH_VS_DENSE."""
    c = af.case_aff_no_rows()
    kw = af.kwargs(c)
    assert c['D'] is None and c['J'] is None and c['Tx'] is None and c['offset'] is not None and c['qf'] is not None
    for s, r in enumerate(af.solve_case(c)[0]):
        X, U = af.lq_condensed(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], q=kw['q'], Pf=kw['Pf'], offset=kw['offset'], qf=kw['qf'])
        e = max(np.abs(r['X'] - X).max() / max(1.0, np.abs(X).max()), np.abs(r['U'] - U).max() / max(1.0, np.abs(U).max()))
        ea = max(np.abs(r['Xa'] - X).max() / max(1.0, np.abs(X).max()), np.abs(r['Ua'] - U).max() / max(1.0, np.abs(U).max()))
        X0, U0 = af.lq_condensed(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], q=kw['q'], Pf=kw['Pf'])
        print('   instance %d: (b) vs dense %.1e, (a) vs dense %.1e after %d iterations; the homogeneous problem differs by %.1e' % (
            s, e, ea, r['a']['iters'], np.abs(U - U0).max()))
        assert r['a']['status'] == 0 and e <= af.AFF_POLISH_VS_DENSE and ea <= af.AFF_IPM_VS_POLISH and np.abs(U - U0).max() > 1e-2


def test_the_loops_of_the_reference():
    """(i) the shifted loop is the deviation loop plus the reference at the phases; (ii) the plant that is not the model; (iii) the push: the hard loop ends
    with status 1 at t*, the soft one goes on, counts a violated row at t* and is back inside afterwards."""
    T = af.T_LOOP
    c = af.loop_shift(); d = c['dev']
    p = c['A'].shape[1]
    ph = (c['k0'] + np.arange(T + 1)) % p
    for s in range(c['X0'].shape[1]):
        L = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], T, **af.kwargs(c))
        Ld = eq.closed_loop_eq(d['A'][0], d['B'][0], d['H'][0], d['N'], d['k0'], d['X0'][0, s], T, **eq.kwargs(d))
        e = max(np.abs(L['X'] - Ld['X'] - c['xref'][0][ph]).max(), np.abs(L['U'] - Ld['U'] - c['uref'][0][ph[:T]]).max())
        print('   (i) instance %d: against the deviation loop plus the reference %.1e, margin %.1e' % (s, e, L['margin']))
        assert L['status'] == 0 and L['certificate'] and L['margin'] >= af.MARGIN_MIN and e <= 100 * af.AFF_SHIFT_VS_DEV
        np.testing.assert_array_equal(L['nact'], Ld['nact'])
    c, plant, W = af.loop_plant()
    for s in range(c['X0'].shape[1]):
        L = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], T, plant=(plant[0][0], plant[1][0]), W=W[0, s], **af.kwargs(c))
        M = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], T, **af.kwargs(c))
        print('   (ii) instance %d: margin %.1e, against the loop on the model %.1e' % (s, L['margin'], np.abs(L['X'] - M['X']).max()))
        assert L['status'] == 0 and L['certificate'] and L['margin'] >= af.MARGIN_MIN and np.abs(L['X'] - M['X']).max() > 1e-2
    c, W, ts = af.loop_push()
    kw = af.kwargs(c)
    hard = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, 0], T, W=W[0, 0], **kw)
    soft = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, 0], T, penalty=np.full(c['d'].shape[1:], af.PUSH_PENALTY), W=W[0, 0], **kw)
    print('   (iii) t* %d: hard status %d after %d steps; soft status %d, x_1 %s, nviol %s' % (ts, hard['status'], hard['steps'], soft['status'],
                                                                                          np.round(soft['X'][:, 0], 4).tolist(), soft['nviol'].tolist()))
    assert ts >= 2 and (np.abs(hard['X'][:ts, 0]) < af.X1_BOUND).all() and abs(hard['X'][ts, 0]) > 2 * af.X1_BOUND
    assert hard['status'] == 1 and hard['steps'] == ts
    assert soft['status'] == 0 and soft['steps'] == T and soft['nviol'][ts] >= 1 and soft['hres'][ts] > af.X1_BOUND
    assert (np.abs(soft['X'][ts + 1:, 0]) <= af.X1_BOUND + 1e-9).all()


def test_a_terminal_right_hand_side_out_of_reach_ends_with_status_1():
    i = af.infeasible_instance()
    P = af.dense_aff(i['A'][0], i['B'][0], i['H'][0], i['N'], i['k0'], i['X0'][0, 0], Pf=i['Pf'][0], Tx='constraint', trhs=i['terminal_rhs'][0])
    a = eq.ipm_eq(P)
    print('   status %d after %d iterations, r_p %.2e' % (a['status'], a['iters'], a['rp']))
    assert i['N'] * i['B'].shape[3] < i['A'].shape[2] and not eq.feasible(P) and a['status'] == 1 and a['iters'] == 60 and a['rp'] > 1e-3


# ----------------------------------------------------------------------------- about_reference
@pytest.mark.parametrize('kind', ['numpy', 'torch'])
@pytest.mark.parametrize('case', [af.case_shift_rows_mixed_small, af.case_shift_soft, af.case_shift_term_box_nu1],
                         ids=['rows_mixed_small', 'soft', 'term_box_nu1'])
def test_about_reference_is_the_shift_of_the_reference_module(case, kind):
    from tunempc_amd import mpc_qp as m
    c = case(); d = c['dev']
    f = (lambda x: x) if kind == 'numpy' else (lambda x: None if x is None or isinstance(x, str) else __import__('torch').from_numpy(np.ascontiguousarray(x)))
    g = (lambda x: x) if kind == 'numpy' else (lambda x: x if isinstance(x, str) else x.numpy())
    tx = d['Tx'] if isinstance(d['Tx'], str) else f(d['Tx'])
    kw = m.about_reference(f(d['A']), f(d['B']), f(d['H']), f(c['xref']), f(c['uref']), q=f(d['q']), Pf=f(d['Pf']), D=f(d['D']), d=f(d['d']), J=f(d['J']), r=f(d['r']),
                           terminal=tx)
    assert set(kw) == {'offset', 'q', 'Pf', 'qf', 'D', 'd', 'terminal', 'terminal_rhs'} | ({'J', 'r'} if d['J'] is not None else set())
    for mine, theirs in (('offset', 'offset'), ('q', 'q'), ('d', 'd'), ('qf', 'qf'), ('terminal_rhs', 'trhs')) + ((('r', 'r'),) if d['J'] is not None else ()):
        np.testing.assert_allclose(g(kw[mine]), c[theirs], rtol=0, atol=1e-14, err_msg=mine)
    assert kw['D'] is not None and g(kw['Pf']) is not None and (isinstance(kw['terminal'], str) or g(kw['terminal']).shape == d['Tx'].shape)
    # a reference that is a trajectory of the model has no offset
    A, B = d['A'], d['B']
    p = A.shape[1]
    if p == 1:
        return
    bare = m.about_reference(A, B, d['H'], c['xref'], c['uref'])
    assert set(bare) == {'offset', 'q'}
    k = np.arange(p)
    np.testing.assert_allclose(bare['offset'], c['xref'][:, (k + 1) % p] - np.einsum('bkij,bkj->bki', A, c['xref']) - np.einsum('bkij,bkj->bki', B, c['uref']), atol=1e-14)


def test_about_reference_refuses_what_it_cannot_shift():
    from tunempc_amd import mpc_qp as m
    z = np.zeros
    A, B, H, xr, ur = z((2, 3, 4, 4)), z((2, 3, 4, 2)), z((2, 3, 6, 6)), z((2, 3, 4)), z((2, 3, 2))
    with pytest.raises(ValueError, match='xref \\(2, 3, 4\\) expected, got \\(2, 3, 3\\)'):
        m.about_reference(A, B, H, xr[..., :3], ur)
    with pytest.raises(ValueError, match='uref \\(2, 3, 2\\) expected'):
        m.about_reference(A, B, H, xr, xr)
    with pytest.raises(ValueError, match='D and d come together'):
        m.about_reference(A, B, H, xr, ur, D=z((2, 3, 1, 6)))
    with pytest.raises(ValueError, match='r describes the rows of J'):
        m.about_reference(A, B, H, xr, ur, r=z((2, 3, 1)))
    with pytest.raises(ValueError, match="terminal must be None, 'constraint' or an array"):
        m.about_reference(A, B, H, xr, ur, terminal='free')
    import torch
    with pytest.raises(ValueError, match='all arguments numpy arrays or all torch tensors'):
        m.about_reference(A, B, H, torch.zeros((2, 3, 4), dtype=torch.float64), ur)


# ----------------------------------------------------------------------------- the interface, without a device
@pytest.fixture
def no_library(monkeypatch):
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_the_affine_arguments_stand_between_the_positional_ones_and_the_keywords_of_the_rows():
    """What comes before the new parameters is where it was (so a positional call keeps its meaning) and penalty, J, r, (necnt,) terminal remain the last ones."""
    from tunempc_amd import mpc_qp as m
    batch = ['phase0', 'D', 'd', 'ndcnt', 'q', 'Pf', 'tol', 'max_iter', 'return_traj']
    one = ['phase0', 'D', 'd', 'q', 'Pf', 'tol', 'max_iter']
    aff, loop = ['offset', 'qf', 'terminal_rhs'], ['plant', 'disturbance']
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(m.mpc_qp_batch) == ['A', 'B', 'H', 'X0', 'horizon'] + batch + aff + ['penalty', 'J', 'r', 'necnt', 'terminal']
    assert names(m.mpc_closed_loop_batch) == ['A', 'B', 'H', 'X0', 'horizon', 'steps'] + batch + aff + loop + ['penalty', 'J', 'r', 'necnt', 'terminal']
    assert names(m.mpc_step) == ['A', 'B', 'Q', 'R', 'N', 'x0', 'horizon'] + one + aff + ['penalty', 'J', 'r', 'terminal']
    assert names(m.mpc_closed_loop_sim) == ['A', 'B', 'Q', 'R', 'N', 'x0', 'horizon', 'steps'] + one + aff + loop + ['penalty', 'J', 'r', 'terminal']
    for f in (m.mpc_qp_batch, m.mpc_closed_loop_batch, m.mpc_step, m.mpc_closed_loop_sim):
        assert all(inspect.signature(f).parameters[k].default is None for k in aff + loop if k in names(f))


def test_the_checks_of_the_affine_arguments_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import mpc_qp as m
    import torch
    z = np.zeros
    A, B, H, X0 = z((2, 3, 4, 4)), z((2, 3, 4, 2)), z((2, 3, 6, 6)), z((2, 5, 4))
    Tx = z((2, 3, 2, 4))
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        with pytest.raises(ValueError, match='offset \\(2, 3, 4\\) expected, got \\(2, 3, 5\\)'):
            f(A, B, H, X0, 3, *extra, offset=z((2, 3, 5)))
        with pytest.raises(ValueError, match='qf \\(2, 3, 4\\) expected, got \\(2, 4\\)'):
            f(A, B, H, X0, 3, *extra, qf=z((2, 4)))
        with pytest.raises(ValueError, match='terminal_rhs describes the rows of terminal, which is None'):
            f(A, B, H, X0, 3, *extra, terminal_rhs=z((2, 3, 4)))
        with pytest.raises(ValueError, match='terminal_rhs \\(2, 3, 2\\) expected, got \\(2, 3, 4\\)'):
            f(A, B, H, X0, 3, *extra, terminal=Tx, terminal_rhs=z((2, 3, 4)))
        with pytest.raises(ValueError, match='terminal_rhs \\(2, 3, 4\\) expected, got \\(2, 3, 2\\)'):
            f(A, B, H, X0, 3, *extra, terminal='constraint', terminal_rhs=z((2, 3, 2)))
        with pytest.raises(ValueError, match='fp64 arrays expected \\(offset has dtype float32\\)'):
            f(A, B, H, X0, 3, *extra, offset=z((2, 3, 4), np.float32))
        with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(qf differs\\)'):
            f(A, B, H, X0, 3, *extra, qf=torch.zeros((2, 3, 4), dtype=torch.float64))
    f = m.mpc_closed_loop_batch
    for bad in ((A,), (A, B, z((2, 3, 4)), A), A, 'model'):
        with pytest.raises(ValueError, match='plant must be \\(Ap, Bp\\) or \\(Ap, Bp, cp\\)'):
            f(A, B, H, X0, 3, 2, plant=bad)
    with pytest.raises(ValueError, match='Ap and Bp come together'):
        f(A, B, H, X0, 3, 2, plant=(A, None))
    with pytest.raises(ValueError, match='plant\\[0\\] \\(2, 3, 4, 4\\) expected, got \\(2, 3, 4, 2\\)'):
        f(A, B, H, X0, 3, 2, plant=(B, B))
    with pytest.raises(ValueError, match='plant\\[1\\] \\(2, 3, 4, 2\\) expected'):
        f(A, B, H, X0, 3, 2, plant=(A, A))
    with pytest.raises(ValueError, match='plant\\[2\\] \\(2, 3, 4\\) expected'):
        f(A, B, H, X0, 3, 2, plant=(A, B, z((2, 3, 3))))
    with pytest.raises(ValueError, match='disturbance \\(2, 5, 2, 4\\) expected, got \\(2, 5, 3, 4\\)'):
        f(A, B, H, X0, 3, 2, disturbance=z((2, 5, 3, 4)))
    with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(disturbance differs\\)'):
        f(A, B, H, X0, 3, 2, disturbance=torch.zeros((2, 5, 2, 4), dtype=torch.float64))
    for name in ('plant', 'disturbance', 'cp', 'W'):                         # the one-step call has no plant
        with pytest.raises(TypeError, match=name):
            m.mpc_qp_batch(A, B, H, X0, 3, **{name: None})
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    with pytest.raises(ValueError, match='mpc_step: offset must be one vector of 2 entries or a list of p = 1 of them'):
        m.mpc_step(*one, offset=np.ones(3))
    with pytest.raises(ValueError, match='mpc_step: terminal_rhs describes the rows of terminal, which is None'):
        m.mpc_step(*one, terminal_rhs=np.ones(2))
    with pytest.raises(ValueError, match='mpc_step: terminal_rhs must be one vector of 1 entries'):
        m.mpc_step(*one, terminal=np.ones((1, 2)), terminal_rhs=np.ones(2))
    with pytest.raises(TypeError, match='plant'):
        m.mpc_step(*one, plant=(np.eye(2), np.ones((2, 1))))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: plant must be a tuple \\(Ap, Bp\\) or \\(Ap, Bp, cp\\)'):
        m.mpc_closed_loop_sim(*one, 3, plant=(np.eye(2),))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: plant\\[1\\] must be one matrix \\[2, 1\\]'):
        m.mpc_closed_loop_sim(*one, 3, plant=(np.eye(2), np.ones((2, 2))))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: disturbance \\[steps, nx\\] = \\[3, 2\\] expected, got \\(2, 2\\)'):
        m.mpc_closed_loop_sim(*one, 3, disturbance=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: qf must be one vector of 2 entries'):
        m.mpc_closed_loop_sim(*one, 3, qf=[np.ones(2), np.ones(2)])


def test_the_layout_did_not_move():
    """The AFF instantiations read c, qf, t, cp, W from global memory: the header has no layout function beyond those of the EQ instantiations."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    assert sorted(set(re.findall(r'inline \w+ (mpc_qp\w*_lds)\(', src))) == ['mpc_qp_eq_lds', 'mpc_qp_lds', 'mpc_qp_soft_lds']
    assert sorted(set(re.findall(r'inline long long (mpc_qp\w*_ws_doubles)\(', src))) == ['mpc_qp_eq_ws_doubles', 'mpc_qp_soft_ws_doubles', 'mpc_qp_ws_doubles']
    assert 'template <bool SOFT, bool EQ, bool AFF>' in src and 'static_assert(EQ || !AFF' in src


def test_the_affine_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_aff_batch_host', 'tmpc_mpc_qp_aff_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 50
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].rstrip().endswith('double* eres, const double* offset,\n' + ' ' * (len(name) + 5) +
                                                         'const double* qf, const double* terminal_rhs, const double* Ap, const double* Bp, const double* cp, const double* W)')


def test_the_affine_entries_refuse_by_themselves_what_python_refuses():
    """TMPC_E_ARG before any device call (this machine may have no device at all): terminal_rhs with nt = 0, Ap without Bp and the other way round; what the eq
    entries refuse stays refused."""
    from tunempc_amd._lib import load_library
    lib = load_library()
    d = (C.c_double * 64)(*([1.0] * 64))
    ok = dict(nb=1, p=2, nx=2, mb=1, nd=1, N=1, ns=1, T=1, k0=0, ne=1, J=d, nt=-1, Tx=None, c=None, qf=None, t=None, Ap=None, Bp=None, cp=None, W=None)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    for f, vp in ((lib.tmpc_mpc_qp_aff_batch_host, False), (lib.tmpc_mpc_qp_aff_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(d), P(d), P(d), None, None, P(d), None, P(d), P(d), 1e-10, 60, P(d), P(d), P(d),
                     None, None, None, None, None, None, None, None, None, None, None, a['ne'], P(a['J']), None, None, a['nt'], P(a['Tx']),
                     None, None, None, P(a['c']), P(a['qf']), P(a['t']), P(a['Ap']), P(a['Bp']), P(a['cp']), P(a['W']))
        assert call(nt=0, t=d) == -1 and b'terminal_rhs describes the terminal rows; got nt = 0' in lib.tmpc_last_error()
        assert call(ne=0, J=None, nt=0, t=d) == -1
        assert call(Ap=d) == -1 and b'Ap without Bp' in lib.tmpc_last_error()
        assert call(Bp=d, c=d) == -1 and b'Bp without Ap' in lib.tmpc_last_error()
        for kw in (dict(ne=-1), dict(J=None), dict(nt=-2, c=d), dict(nt=1, c=d), dict(nb=0, W=d)):
            assert call(**kw) == -1, kw
        assert call(nt=3, Tx=d, t=d) == -2 and b'at most nx = 2 terminal rows' in lib.tmpc_last_error()
