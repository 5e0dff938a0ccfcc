"""The numpy reference of the local gain of a solved MPC step (tests/mpc_qp_gain_reference.py), the argument checks of the two new C entries and of the
Python wrappers; no GPU is needed.

Method (a) (the constraint-to-go recursion on the per-instance expanded data) against method (b) (central differences, h = 1e-4, of the polished active-set
solution) times Pz_0, K_0 and the open-loop sensitivities, relative to max(1, max|.|).  Measured here, worst instance per case (every figure is printed):
    case_box_nu1 4.3e-12, case_box_nu2 2.2e-12, case_mixed_small 2.0e-11, case_single_phase 3.1e-12 (small shapes: <= 2.1e-11),
    case_box_bench 6.9e-11, case_mixed_bench 4.4e-10 (bench shapes, up to 4 active rows in a stage and 9 in the horizon),
    case_state_box 5.8e-11 (cnt = [0, 1, 1, 0], two active rows at a stage of two inputs).
In every run the active set is unchanged at +-h, strict = 1.000000 and the polish certificate holds, so no instance is skipped.  The assertion stands at ten
times these figures (mpc_qp_gain_reference.AB_MEASURED).  (a) against the dense null-space solve (c): <= 5.5e-15 everywhere; the GPU tests hold two GPU paths
of one stage to ten times that figure of the case, with a floor of 1e-13.  The certificate on the state-box case: dK0_rel <= 4.0e-16, du0 <= 9.9e-14."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lqr_horizon_reference as lh
import mpc_qp_reference as mq
import mpc_qp_eq_reference as eqr
import mpc_qp_soft_reference as ms
import mpc_qp_quad_reference as mqq
import mpc_qp_gain_reference as gr

CASES = [mq.case_box_nu1, mq.case_box_nu2, mq.case_mixed_small, mq.case_single_phase, mq.case_box_bench, mq.case_mixed_bench, gr.case_state_box]


# ----------------------------------------------------------------------------- (a) against (b)
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.__name__)
def test_recursion_against_finite_differences_of_the_polished_solution(case):
    insts = gr.hard_instances(case)
    worst = 0.0
    for s, (i, r) in enumerate(zip(insts, gr.solved(case.__name__, insts))):
        g, cls, strict = gr.gain_of_instance(i, r)
        fd = gr.fd_gain(i, r, g['Pz0'])
        dX, dU = gr.sensitivities(g['E'], g, i['N'])
        ek, es = gr.rel(g['K0'], fd['K0']), max(gr.rel(dX, fd['dX']), gr.rel(dU, fd['dU']))
        print('%s[%d]: active per stage %s, cnt %s, strict %.6f, margin %.1e, K0 %.2e, sensitivities %.2e' % (
            case.__name__, s, cls.sum(axis=1).tolist(), g['cnt'].tolist(), strict, r['b']['margin'], ek, es))
        assert r['a']['status'] == 0 and r['b']['certificate'] and fd['certificate'] and strict >= 0.999 and not g['infeasible']
        assert g['feas'] <= 1e-10
        worst = max(worst, ek, es)
    print('%s: worst %.2e, asserted at %.1e' % (case.__name__, worst, gr.ab_bound(case)))
    assert worst <= gr.ab_bound(case)


def test_state_box_case_is_what_it_says():
    c = gr.case_state_box()
    insts = gr.hard_instances(gr.case_state_box)
    sol = gr.solved('case_state_box', insts)
    assert c['N'] == 4 and c['k0'] == 1 and np.array_equal(np.abs(c['X0'][..., 0]), np.full((1, 4), 0.1))
    cnts = [gr.gain_of_instance(i, r)[0]['cnt'].tolist() for i, r in zip(insts, sol)]
    acts = [gr.gain_of_instance(i, r)[1].sum(axis=1).tolist() for i, r in zip(insts, sol)]
    assert [0, 1, 1, 0] in cnts and any(max(a) == 2 for a in acts)           # active state rows; two active rows at a stage of two inputs


def test_recursion_is_the_horizon_pass_on_expanded_data_and_agrees_with_the_dense_solve():
    for case in CASES:
        k = gr.kkt_disagreement(case)
        print('%s: (a) against (c) %.2e' % (case.__name__, k))
        assert k <= 1e-13
    # without active rows the expanded pass is the horizon pass of the periodic model
    c = mq.case_box_nu1()
    g = gr.gain(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], np.zeros((c['N'], 2), int), c['D'][0], None, c['Pf'][0])
    r = lh.horizon_lqr(c['A'][0], c['B'][0], c['H'][0], None, None, c['N'], c['k0'], 'cost', c['Pf'][0])
    assert gr.rel(g['K0'], r['K0']) <= 1e-14 and gr.rel(g['Pi0'], r['Pi0']) <= 1e-14


def test_per_instance_figures_of_the_dense_solve_are_the_stored_ones():
    """(a) against (c) per instance, at the rule's active set and with every row free: what the GPU tests take their two-paths bound from."""
    for name, stored in gr.KKT_MEASURED.items():
        case = {c.__name__: c for c in CASES}[name]
        got, free = gr.kkt_instances(case), gr.kkt_free(case)
        print('%s: per instance %s (stored %s), every row free %.2e (stored %.1e)' % (name, ['%.2e' % x for x in got], stored, free, gr.KKT_FREE_MEASURED[name]))
        assert len(got) == len(stored) and all(g <= 10 * s for g, s in zip(got, stored)) and free <= 10 * gr.KKT_FREE_MEASURED[name]
        assert all(gr.two_paths_bound(case, s) == gr.KKT_FLOOR for s in range(len(got)))      # (ten times every figure lies below the floor today)


@pytest.mark.parametrize('case', [eqr.case_term_box_nu2, eqr.case_tx_box_nu2, eqr.case_rows_mixed_small], ids=lambda c: c.__name__)
def test_terminal_and_equality_rows_against_finite_differences_of_their_own_polished_solution(case):
    """x_N = 0, a Tx with nt = 2 < nx = 3 (the start Hn_N of `_pass`), ragged J rows with terminal rows: method (a) against central differences of
    mpc_qp_eq_reference.polish_eq, a dense KKT solve that shares no stage algebra with the recursion.  Measured: 2.3e-12, 2.3e-12, 2.0e-11."""
    c = case()
    worst = 0.0
    for s, r in enumerate(eqr.solve_case(c)[0]):
        g, cls, strict = gr.gain_of_eq_instance(c, 0, s, r)
        fd = gr.fd_gain_eq(c, 0, s, r, g['Pz0'])
        e = gr.rel(g['K0'], fd['K0'])
        print('%s[%d]: active per stage %s, cnt %s, strict %.6f, K0 %.2e' % (case.__name__, s, cls.sum(axis=1).tolist(), g['cnt'].tolist(), strict, e))
        assert r['a']['status'] == 0 and r['b']['certificate'] and fd['certificate'] and strict >= 0.999 and not g['infeasible']
        worst = max(worst, e)
    assert worst <= 10 * gr.AB_EQ_MEASURED[case.__name__]


# ----------------------------------------------------------------------------- the certificate on the reference
def test_certificate_on_the_state_box_case():
    """H, P of the case: the economic side carries Pf + P[(k0 + N) mod p].  The interior-point reference converges on the indefinite H with the active set of
    the Hc side, and the gains of both sides at that set agree."""
    c = gr.case_state_box()
    insts = gr.hard_instances(gr.case_state_box)
    worst = 0.0
    for i, r in zip(insts, gr.solved('case_state_box', insts)):
        gC, cls, strict = gr.gain_of_instance(i, r)
        kw = dict(i['kw']); kw['Pf'] = c['Pf'][0] + c['P'][0]
        iH = dict(i, H=c['Hecon'][0], kw=kw)
        rH = gr.solve_instance(iH)
        gH, clsH, _ = gr.gain_of_instance(iH, rH, cls=cls)
        same = np.array_equal(gr.gain_of_instance(iH, rH)[1], cls)
        dk, du = gr.rel(gH['K0'], gC['K0']), np.abs(rH['U'][0] - r['U'][0]).max()
        print('state box: status of the H side %d, same active set %s, dK0_rel %.2e, du0 %.2e, subspace %.2e' % (
            rH['a']['status'], same, dk, du, np.abs(gH['Pz0'] - gC['Pz0']).max()))
        assert rH['a']['status'] == 0 and same and rH['b']['certificate']
        assert dk <= 1e-12 and du <= 1e-12 and np.abs(gH['Pz0'] - gC['Pz0']).max() <= 1e-12
        worst = max(worst, dk)
    assert worst <= 1e-12


# ----------------------------------------------------------------------------- soft and quadratic rows
def test_a_violated_l1_row_leaves_the_gain_of_the_problem_without_it():
    i = ms.infeasible_instance()                                             # rows +-x_1 <= 0.1 with c = 50, x_0 far outside: violated rows along the horizon
    r = gr.solve_instance(i)
    g, cls, strict = gr.gain_of_instance(i, r)
    st = r['State']
    assert r['b']['certificate'] and strict >= 0.999 and (st == mqq.VIOLATED).any()
    assert not cls[st == mqq.VIOLATED].any() and np.array_equal(cls == 1, st == mqq.ACTIVE)
    free = gr.gain(i['A'], i['B'], i['H'], i['N'], i['k0'], np.where(st == mqq.VIOLATED, 0, cls), i['kw']['D'], None, i['kw']['Pf'])
    fd = gr.fd_gain(i, r, g['Pz0'])
    print('violated L1 rows %d, active %d: against FD %.2e' % ((st == mqq.VIOLATED).sum(), (cls == 1).sum(), gr.rel(g['K0'], fd['K0'])))
    assert fd['certificate'] and gr.rel(g['K0'], fd['K0']) <= 1e-9 and np.array_equal(g['K0'], free['K0'])
    if not (cls == 1).any():                                                 # nothing else is active: the unconstrained law
        u = lh.horizon_lqr(i['A'], i['B'], i['H'], None, None, i['N'], i['k0'], 'cost', i['kw']['Pf'])
        assert gr.rel(g['K0'], u['K0']) <= 1e-13


def test_an_active_pure_quadratic_row_gives_the_gain_of_h_plus_z_dd():
    i = mqq.infeasible_instance(0.0, 500.0)
    r = gr.solve_instance(i)
    g, cls, strict = gr.gain_of_instance(i, r)
    assert r['b']['certificate'] and strict >= 0.999 and (cls == 2).any() and not (cls == 1).any()
    p, n = i['A'].shape[0], i['H'].shape[1]
    # the same pass spelled out: no rows, Z D'D of the active rows in a per-stage Hessian
    E = gr.expand(i['A'], i['B'], i['H'], i['N'], i['k0'], np.zeros_like(cls))
    for j in range(i['N']):
        k = (i['k0'] + j) % p
        for q in np.flatnonzero(cls[j] == 2):
            E['H'][j] += 500.0 * np.outer(i['kw']['D'][k, q], i['kw']['D'][k, q])
    Pn = i['kw']['Pf'][(i['k0'] + i['N']) % p]
    u = lh.horizon_lqr(E['A'], E['B'], E['H'], None, None, i['N'], 0, 'cost', np.array([Pn] * i['N']))
    fd = gr.fd_gain(i, r, g['Pz0'])
    print('active pure rows %d: against FD %.2e, against the spelled-out pass %.2e' % ((cls == 2).sum(), gr.rel(g['K0'], fd['K0']), gr.rel(g['K0'], u['K0'])))
    assert fd['certificate'] and gr.rel(g['K0'], fd['K0']) <= 1e-9 and gr.rel(g['K0'], u['K0']) <= 1e-13
    # an inactive pure row (x_0 inside the bound) is class 0
    i2 = dict(i, x0=0.05 * i['x0'] / np.abs(i['x0']).max())
    r2 = gr.solve_instance(i2)
    assert not gr.gain_of_instance(i2, r2)[1].any()


# ----------------------------------------------------------------------------- the C ABI and the host-side argument checks (no device needed)
NAMES = ('tmpc_mpc_qp_gain_batch_host', 'tmpc_mpc_qp_gain_batch_device')


def test_the_gain_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 40


def _raw(name, **over):
    """The entry called directly with small valid arguments (host arrays for both entries: a refused call touches none of them), some replaced."""
    from tunempc_amd._lib import load_library
    lib = load_library()
    a = dict(nb=1, p=2, nx=3, mb=2, nd=2, ne=0, nt=0, N=3, ns=1, k0=0, terminal=0, rank_tol=1e-9, null=())
    a.update(over)
    buf = np.zeros(1 << 16)
    ibuf = np.zeros(1 << 12, np.int32)
    host = name.endswith('host')
    dp = (lambda: buf.ctypes.data_as(C.POINTER(C.c_double))) if host else (lambda: C.c_void_p(buf.ctypes.data))
    ip = (lambda: ibuf.ctypes.data_as(C.POINTER(C.c_int32))) if host else (lambda: C.c_void_p(ibuf.ctypes.data))
    order = [('A', dp), ('B', dp), ('H', dp), ('Pf', None), ('D', dp), ('ndcnt', None), ('d', dp), ('penalty', None), ('penalty2', None), ('J', None),
             ('necnt', None), ('Tx', None), ('X', dp), ('U', dp), ('Lam', dp), ('Eps', None), ('cls_in', None)]
    outs = [('K0', dp), ('Pi0', dp), ('Hn0', dp), ('cnt0', ip), ('info', dp), ('cls', None), ('strict', None), ('Kall', None), ('cntall', None), ('dX', None),
            ('dU', None)]
    val = lambda nm, f: a[nm]() if callable(a.get(nm)) else (None if f is None or nm in a['null'] else f())
    args = [a[k] for k in ('nb', 'p', 'nx', 'mb', 'nd', 'ne', 'nt', 'N', 'ns', 'k0', 'terminal')] + [val(nm, f) for nm, f in order] + [a['rank_tol']]
    args += [val(nm, f) for nm, f in outs]
    rc = getattr(lib, name)(*args)
    return rc, lib.tmpc_last_error().decode(), dp


@pytest.mark.parametrize('name', NAMES)
def test_the_entries_check_their_arguments_before_any_device_call(name):
    for over, code, text in ((dict(nb=0), -1, 'bad argument'), (dict(N=0), -1, 'bad argument'), (dict(null=('X',)), -1, 'non-null A, B, H, X, U'),
                             (dict(null=('K0',)), -1, 'bad argument'), (dict(k0=2), -1, 'k0 = 2 outside 0 .. p - 1 = 1'), (dict(terminal=3), -1, 'terminal 0'),
                             (dict(terminal=2), -1, 'non-null Tx, nt >= 1'), (dict(null=('Lam',)), -1, 'non-null D, d, Lam when nd = 2'),
                             (dict(ne=1), -1, 'non-null J when ne = 1'), (dict(rank_tol=0.0), -1, 'finite rank_tol > 0'),
                             (dict(nx=40, mb=30), -2, 'stage blocks up to nx \\+ nu = 64'), (dict(nx=32, mb=32, nd=40), -2, 'bytes of LDS \\(limit 163840\\)'),
                             (dict(nb=70000), -2, 'at most 65535 problems')):
        rc, msg, _ = _raw(name, **over)
        assert rc == code and msg.startswith(name + ': ') and re.search(text, msg), (over, rc, msg)
    rc, msg, dp = _raw(name)
    rc, msg, _ = _raw(name, terminal=2, nt=4, Tx=dp)
    assert rc == -2 and msg.startswith(name + ': ') and re.search('at most nx = 3 terminal rows \\(got nt = 4\\)', msg)
    rc, msg, _ = _raw(name, dX=dp)
    assert rc == -1 and 'dX and dU come together and need Kall' in msg
    rc, msg, _ = _raw(name, penalty2=dp)
    assert rc == -1 and 'penalty2 stands beside penalty' in msg


def _sol(nb=1, ns=2, p=2, nx=3, nu=2, nd=2, N=3):
    A, B, H = np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, nu)), np.tile(np.eye(nx + nu), (nb, p, 1, 1))
    sol = dict(X=np.zeros((nb, ns, N + 1, nx)), U=np.zeros((nb, ns, N, nu)), lam=np.zeros((nb, ns, N, nd)), eps=np.zeros((nb, ns, N, nd)))
    return A, B, H, sol, dict(D=np.zeros((nb, p, nd, nx + nu)), d=np.ones((nb, p, nd)))


def test_the_wrappers_check_their_arguments_before_any_device_call():
    import torch
    from tunempc_amd import mpc_qp as m
    A, B, H, sol, rows = _sol()
    with pytest.raises(ValueError, match='mpc_qp_gain_batch: sol must be a dict'):
        m.mpc_qp_gain_batch(A, B, H, None, 3, **rows)
    with pytest.raises(ValueError, match="sol\\['X'\\] \\[nb, ns, horizon \\+ 1, nx\\] expected"):
        m.mpc_qp_gain_batch(A, B, H, dict(sol, X=None), 3, **rows)
    with pytest.raises(ValueError, match="sol\\['lam'\\] \\(1, 2, 3, 2\\) expected, got None"):
        m.mpc_qp_gain_batch(A, B, H, dict(sol, lam=None), 3, **rows)
    with pytest.raises(ValueError, match="sol\\['U'\\] \\(1, 2, 3, 2\\) expected, got \\(1, 2, 4, 2\\)"):
        m.mpc_qp_gain_batch(A, B, H, dict(sol, U=np.zeros((1, 2, 4, 2))), 3, **rows)
    with pytest.raises(ValueError, match="sol\\['eps'\\] .* expected, got None"):
        m.mpc_qp_gain_batch(A, B, H, dict(sol, eps=None), 3, penalty=np.ones((1, 2, 2)), **rows)
    with pytest.raises(ValueError, match='horizon must be an int >= 1'):
        m.mpc_qp_gain_batch(A, B, H, sol, 0, **rows)
    with pytest.raises(ValueError, match='0 < rank_tol < 1 expected'):
        m.mpc_qp_gain_batch(A, B, H, sol, 3, rank_tol=1.0, **rows)
    with pytest.raises(ValueError, match='active int32 \\(1, 2, 3, 2\\) expected'):
        m.mpc_qp_gain_batch(A, B, H, sol, 3, active=np.zeros((1, 2, 3, 2)), **rows)
    with pytest.raises(ValueError, match='active in 0 \\(free\\), 1 \\(equality\\), 2 \\(quadratic\\) expected, got 0 .. 3'):
        m.mpc_qp_gain_batch(A, B, H, sol, 3, active=np.full((1, 2, 3, 2), 3, np.int32) * np.eye(2, dtype=np.int32)[0], **rows)
    with pytest.raises(ValueError, match='active describes the rows of D, which is None'):
        m.mpc_qp_gain_batch(A, B, H, sol, 3, active=np.zeros((1, 2, 3, 0), np.int32))
    with pytest.raises(ValueError, match='all numpy arrays or all torch tensors'):
        m.mpc_qp_gain_batch(A, B, H, dict(sol, U=torch.zeros((1, 2, 3, 2), dtype=torch.float64)), 3, **rows)
    with pytest.raises(ValueError, match='D and d come together'):
        m.mpc_qp_gain_batch(A, B, H, sol, 3, D=rows['D'])
    with pytest.raises(NotImplementedError, match='mpc_qp_gain_batch: nx = 20, nu = 4 with room for 0 \\+ 330 rows per stage and a constraint-to-go needs \\d+ bytes'):
        A2, B2, H2, sol2, rows2 = _sol(nx=20, nu=4, nd=330)
        m.mpc_qp_gain_batch(A2, B2, H2, sol2, 3, **rows2)
    with pytest.raises(ValueError, match='mpc_gain_equivalence_batch: without terminal rows .* P is needed'):
        m.mpc_gain_equivalence_batch(A, B, H, H, sol['X'][:, :, 0], 3, **rows)
    with pytest.raises(ValueError, match='mpc_gain_equivalence_batch: Hc .* expected'):
        m.mpc_gain_equivalence_batch(A, B, H, H[:, :, :4, :4], sol['X'][:, :, 0], 3, P=A, **rows)
    with pytest.raises(ValueError, match='mpc_step_gain: sol must be a dict'):
        m.mpc_step_gain(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), None, 3)


def test_the_layout_restated_in_python_is_the_layout_of_the_horizon_entry_plus_the_classes():
    from tunempc_amd import mpc_qp as m
    assert m.gain_lds_bytes(24, 8, 16, 0) <= m.LDS_BYTES and m.gain_lds_bytes(24, 8, 0, 0) + 8 * 17 < m.gain_lds_bytes(24, 8, 16, 0)
    assert m.gain_lds_bytes(3, 2, 0, 0) == 8 * (3 * 7 + 3 * 3 + 4 * 7 + 7 * 7 + 2 * 3 * 5 + 2 * 3 * 3 + 16 + 1)
