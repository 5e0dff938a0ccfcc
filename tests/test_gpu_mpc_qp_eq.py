"""GPU tests of the MPC step with equality rows and a terminal constraint (the EQ instantiations of csrc/tmpc_mpc_qp.h, tunempc_amd.mpc_qp with J=, r=, necnt=,
terminal=) against method (b) of tests/mpc_qp_eq_reference.py (the polished solution with its optimality certificate), through the host and the device entry.

Bounds.  Against the reference: PARITY = 10 x EQ_IPM_VS_POLISH, ten times what the numpy iteration reaches against the same truth (test_mpc_qp_eq_cpu.py, where
it is asserted); u0, X, U relative to max(1, max|.|), lam, nu, nu_term and the slacks relative to max(1, max lam, max|nu|).  Against the fixed-active-set law of
horizon_lqr_batch: 10 x EQ_POLISH_VS_LQR.  Bit-identity where the kernel promises it.  Iteration counts are printed, not compared."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_eq_reference as eq  # noqa: E402

PARITY = 10 * eq.EQ_IPM_VS_POLISH
LAW = 10 * eq.EQ_POLISH_VS_LQR
ENTRIES = ['host', 'device']
T_LOOP = 7
OUT_KEYS = ('u0', 'X', 'U', 'lam', 'nact', 'hres', 'x1', 'info')
EQ_KEYS = ('nu', 'nu_term', 'eres')
LOOP_KEYS = ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def run(entry, bt, steps=None, **kw):
    """mpc_qp_batch (steps None) or mpc_closed_loop_batch on a batch dict of mpc_qp_eq_reference.batch_of -> dict of numpy arrays."""
    from tunempc_amd import mpc_qp as m
    f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
    opt = {k: f(bt[k]) for k in ('D', 'd', 'ndcnt', 'q', 'Pf', 'penalty', 'J', 'r', 'necnt') if bt.get(k) is not None}
    if bt.get('terminal') is not None:
        opt['terminal'] = bt['terminal'] if isinstance(bt['terminal'], str) else f(bt['terminal'])
    args = (f(bt['A']), f(bt['B']), f(bt['H']), f(bt['X0']), bt['N'])
    out = m.mpc_qp_batch(*args, bt['k0'], **opt, **kw) if steps is None else m.mpc_closed_loop_batch(*args, steps, bt['k0'], **opt, **kw)
    return to_host(out)


def assert_same(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def members(bt, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in bt.items()}


def keys_of(bt, base):
    return base + (('eps', 'nviol') if bt.get('penalty') is not None else ())


# ----------------------------------------------------------------------------- 1. the open-loop solution against method (b), and by itself
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', eq.VALUE_CASES, ids=[c.__name__ for c in eq.VALUE_CASES])
def test_open_loop_solution_against_the_polished_solution(entry, case):
    from tunempc_amd import mpc_qp as m
    c = case()
    ref = eq.solve_case(c)
    out = run(entry, eq.batch_of(c))
    soft = c['penalty'] is not None
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == 1).all()
    assert (out['iters_total'] <= m.MAX_ITER).all() and (out['pivmin'] > 0).all()
    for b, rb in enumerate(ref):
        kw = eq.kwargs(c, b)
        for s, r in enumerate(rb):
            o = {k: out[k][b, s] for k in ('u0', 'X', 'U', 'lam', 'nu', 'nu_term', 'nact', 'eres') + (('eps', 'nviol') if soft else ())}
            ms = eq.mult_scale(r)
            e = dict(u0=relmax(o['u0'], r['U'][0]), X=relmax(o['X'], r['X']), U=relmax(o['U'], r['U']), lam=np.abs(o['lam'] - r['Lam']).max() / ms if r['Lam'].size else 0.0,
                     nu=np.abs(o['nu'] - r['Nu']).max() / ms if r['Nu'].size else 0.0, nu_term=np.abs(o['nu_term'] - r['NuT']).max() / ms if r['NuT'].size else 0.0)
            if soft:
                e['eps'] = np.abs(o['eps'] - r['Eps']).max() / ms
            k = eq.kkt_check_eq(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], o['X'], o['U'], o['lam'], o['nu'], o['nu_term'], o.get('eps'),
                                None if not soft else c['penalty'][b], **kw)
            print('   %s %s instance %d.%d: iters %d (numpy %d) mu %.1e | vs (b) %s | by itself %s' % (
                entry, c['name'], b, s, out['iters_total'][b, s], r['a']['iters'], out['mu'][b, s], {q: '%.1e' % v for q, v in e.items()}, {q: '%.1e' % v for q, v in k.items()}))
            assert r['b']['certificate'] and r['b']['margin'] >= eq.MARGIN_MIN
            assert max(e.values()) <= PARITY, e
            assert o['nact'] == r['nact0'] and (not soft or o['nviol'] == r['nviol0'])
            assert abs(o['eres'] - r['eres0']) <= PARITY and o['eres'] <= PARITY * max(1.0, 0.0 if c['r'] is None else np.abs(c['r']).max())
            assert max(k['dyn'], k['eq'], k['term'], k['comp'], k['comp_e'], k['stat']) <= PARITY and k['viol'] <= PARITY and k['lam_min'] >= -PARITY * ms, k
    assert out['nu'].shape == out['X'].shape[:2] + (c['N'], 0 if c['J'] is None else c['J'].shape[2])
    assert out['nu_term'].shape == out['X'].shape[:2] + (c['A'].shape[2] if isinstance(c['Tx'], str) else c['Tx'].shape[2],)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_dependent_equality_row_changes_the_solution_by_rounding(entry):
    dep, one = eq.case_dependent_row(), eq.case_rows_mixed_small()
    out = run(entry, eq.batch_of(dep))
    assert not out['status'].any()
    for s, r in enumerate(eq.solve_case(one)[0]):
        e = dict(u0=relmax(out['u0'][0, s], r['U'][0]), X=relmax(out['X'][0, s], r['X']), U=relmax(out['U'][0, s], r['U']),
                 lam=np.abs(out['lam'][0, s] - r['Lam']).max() / eq.mult_scale(r))
        print('   %s instance %d: iters %d | vs (b) of the row stated once %s' % (entry, s, out['iters_total'][0, s], {q: '%.1e' % v for q, v in e.items()}))
        assert max(e.values()) <= PARITY and out['eres'][0, s] <= PARITY


# ----------------------------------------------------------------------------- 2. against the fixed-active-set law (the other GPU kernel)
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('which', eq.LQR_CASES)
def test_without_inequality_rows_the_step_is_the_law_of_horizon_lqr_batch(entry, which):
    from tunempc_amd import lqr
    c = eq.case_lqr(which)
    bt = eq.batch_of(c)
    out = run(entry, bt)
    f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
    law = to_host(lqr.horizon_lqr_batch(f(c['A']), f(c['B']), f(c['H']), c['N'], terminal='constraint', Pf=f(c['Pf']), phases=[c['k0']], J=f(c['J']), ncnt=f(bt['necnt'])))
    assert not out['status'].any() and not law['status'].any() and (law['cnt0'] == 0).all()
    u = -np.einsum('ux,sx->su', law['K0'][0, 0], c['X0'][0])
    e = np.abs(out['u0'][0] - u).max() / max(1.0, np.abs(u).max())
    print('   %s %s: iters %s | u0 against -K0 x0 %.1e, |x_N| %.1e, eres %.1e' % (entry, which, out['iters_total'][0].tolist(), e, np.abs(out['X'][0, :, -1]).max(),
                                                                             out['eres'].max()))
    assert e <= LAW and np.abs(out['X'][0, :, -1]).max() <= PARITY and out['eres'].max() <= PARITY
    assert out['lam'].shape[-1] == 0 and (out['nact'] == 0).all() and np.isneginf(out['hres']).all()


# ----------------------------------------------------------------------------- 3. the closed loop over T = 7 against the loop on method (b)
LOOP_CASES = eq.SMALL + [eq.case_term_box_bench]


@functools.lru_cache(maxsize=None)
def loop_reference(case):
    c = case()
    return [[eq.closed_loop_eq(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, T_LOOP, None if c['penalty'] is None else c['penalty'][b], **eq.kwargs(c, b))
             for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', LOOP_CASES, ids=[c.__name__ for c in LOOP_CASES])
def test_closed_loop_against_the_loop_on_the_polished_solution(entry, case):
    c = case()
    bt = eq.batch_of(c)
    ref = loop_reference(case)
    out = run(entry, bt, T_LOOP)
    nb, ns = c['X0'].shape[:2]
    assert out['eres'].shape == (nb, ns, T_LOOP) and not out['status'].any() and (out['steps'] == T_LOOP).all()
    rmax = max(1.0, 0.0 if c['r'] is None else np.abs(c['r']).max())
    for b in range(nb):
        for s, r in enumerate(ref[b]):
            assert r['certificate'] and r['margin'] >= eq.MARGIN_MIN, (b, s, r['margin'])
            fin = np.isfinite(r['hres'])
            e = dict(X=relmax(out['X'][b, s], r['X']), U=relmax(out['U'][b, s], r['U']), hres=relmax(out['hres'][b, s][fin], r['hres'][fin]),
                     eres=np.abs(out['eres'][b, s] - r['eres']).max())
            print('   %s %s instance %d.%d: iters %s nact %s eres %.1e | %s' % (entry, c['name'], b, s, out['iters'][b, s].tolist(), out['nact'][b, s].tolist(),
                                                                            out['eres'][b, s].max(), {q: '%.1e' % v for q, v in e.items()}))
            assert max(e.values()) <= PARITY, e
            assert (out['eres'][b, s] <= PARITY * rmax).all()
            np.testing.assert_array_equal(out['nact'][b, s], r['nact'])
            if c['penalty'] is not None:
                np.testing.assert_array_equal(out['nviol'][b, s], r['nviol'])
            np.testing.assert_array_equal(np.isneginf(out['hres'][b, s]), ~fin)
    one = run(entry, bt)
    np.testing.assert_array_equal(one['u0'], out['u0']); np.testing.assert_array_equal(one['eres'], out['eres'][:, :, 0])
    short = run(entry, bt, T_LOOP, return_traj=False)
    assert short['X'] is None and short['U'] is None
    assert_same(short, out, [k for k in keys_of(bt, LOOP_KEYS + ('eres',)) if k not in ('X', 'U', 'eps')])


# ----------------------------------------------------------------------------- 4. the point of the rows
@pytest.mark.parametrize('case', [eq.case_term_p1, eq.case_term_box_nu2], ids=['term_p1', 'term_box_nu2'])
def test_the_terminal_constraint_is_met_and_changes_the_first_input(case):
    c = case()
    bt = eq.batch_of(c)
    con, free = run('device', bt), run('device', dict(bt, terminal=None))
    assert not con['status'].any() and not free['status'].any() and 'nu_term' not in free
    act = [s for s in range(c['X0'].shape[1]) if (con['lam'][0, s] > eq.MARGIN_MIN / 2).any()]
    assert act
    for s in act:
        du, xc, xf = np.abs(con['u0'][0, s] - free['u0'][0, s]).max(), np.abs(con['X'][0, s, -1]).max(), np.abs(free['X'][0, s, -1]).max()
        print('   instance %d: |x_N| %.1e with the constraint, %.2e with the terminal weight alone, |du_0| %.2e' % (s, xc, xf, du))
        assert du > 1e-2 and xc <= PARITY and xf > 1e-2


# ----------------------------------------------------------------------------- 5. bit-identity
@pytest.mark.parametrize('case', [mq.case_mixed_small, mq.case_box_bench], ids=['mixed_small', 'box_bench'])
def test_without_the_new_rows_the_call_is_the_existing_one_bit_for_bit(case):
    """J=None, terminal=None through the keywords, and ne = 0 / nt = 0 through the new C entries, against the calls without them: hard and soft."""
    from tunempc_amd import _lib
    c = case()
    bt = dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=c['rows'].astype(np.int32), N=c['N'], k0=c['k0'])
    pen = np.full(c['d'].shape, 0.3)
    for entry in ENTRIES:
        f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
        for penalty in (None, pen):
            b2 = dict(bt, penalty=penalty)
            plain = run(entry, b2); kw = run(entry, dict(b2, J=None, r=None, necnt=None, terminal=None))
            assert_same(plain, kw, keys_of(b2, OUT_KEYS))
            assert 'nu' not in kw and 'eres' not in kw
            plainT = run(entry, b2, T_LOOP)
            fn = _lib.mpc_qp_eq_batch_device if entry == 'device' else _lib.mpc_qp_eq_batch_host
            old = (_lib.mpc_qp_soft_batch_device if entry == 'device' else _lib.mpc_qp_soft_batch_host) if penalty is not None else \
                (_lib.mpc_qp_batch_device if entry == 'device' else _lib.mpc_qp_batch_host)
            a = [f(b2[k]) for k in ('A', 'B', 'H', 'q', 'Pf', 'D', 'ndcnt', 'd')]
            new = to_host(fn(*a, f(penalty), None, None, None, None, f(b2['X0']), c['N'], T_LOOP, c['k0'], 1e-10, 60, True, False))
            ref = to_host(old(*a, *(() if penalty is None else (f(penalty),)), f(b2['X0']), c['N'], T_LOOP, c['k0'], 1e-10, 60, True, False))
            assert_same(new, ref, ('U0', 'XT', 'info', 'X', 'U', 'iters', 'nact', 'hres') + (('nviol',) if penalty is not None else ()))
            assert (new['eres'] == 0).all() and new['eres'].shape == ref['hres'].shape
            np.testing.assert_array_equal(new['X'], plainT['X'])


@pytest.mark.parametrize('case', [eq.case_rows_mixed_small, eq.case_term_box_bench, eq.case_soft], ids=['rows_mixed_small', 'term_box_bench', 'soft'])
def test_entries_neighbours_and_absent_outputs_do_not_change_a_bit(case):
    c = case()
    bt = eq.batch_of(c)
    keys = keys_of(bt, LOOP_KEYS + ('eres',))
    keys = tuple(k for k in keys if k != 'eps')
    dev = run('device', bt, T_LOOP); host = run('host', bt, T_LOOP)
    assert not dev['status'].any()
    assert_same(dev, host, keys)
    assert_same(run('device', bt), run('host', bt), keys_of(bt, OUT_KEYS + EQ_KEYS))
    ns = bt['X0'].shape[1]
    for s in range(min(ns, 3)):
        for width in (1, 2, 3):
            part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, s:s + width])), T_LOOP)
            for k in keys:
                np.testing.assert_array_equal(part[k][:, 0], dev[k][:, s], err_msg='%s of state %d in a call of %d' % (k, s, width))
    full = run('device', bt); short = run('device', bt, return_traj=False)
    assert short['X'] is None and short['U'] is None and short['lam'] is None and short['nu'] is None and short['nu_term'] is None
    assert_same(short, full, [k for k in keys_of(bt, OUT_KEYS + ('eres',)) if k not in ('X', 'U', 'lam', 'eps')])


def scalar_batch(x0s):
    """nx = nu = 1, N = 2, the box |u| <= 0.6 and x_2 = 0: every |x_0| <= 0.6 (0.7 + 0.7 0.9) / 0.81 is feasible."""
    a, b = 0.9, 0.7
    D = np.array([[[[0.0, 1.0], [0.0, -1.0]]]])
    return dict(A=np.array([[[[a]]]]), B=np.array([[[[b]]]]), H=np.array([[[[2.0, 0.3], [0.3, 1.5]]]]), Pf=np.array([[[[1.2]]]]), D=D, d=np.full((1, 1, 2), 0.6),
                X0=np.asarray(x0s, float).reshape(1, -1, 1), N=2, k0=0, q=None, ndcnt=None, terminal='constraint')


def test_more_instances_than_workspace_slots():
    from tunempc_amd import mpc_qp as m
    ns = m.SLOTS + 37
    x0s = np.linspace(-0.9, 0.9, ns)
    bt = scalar_batch(x0s)
    full = run('device', bt, 3)
    assert not full['status'].any() and (full['nact'][0, :, 0] == 1).any() and (full['nact'][0, :, 0] == 0).any()
    for lo in range(0, ns, m.SLOTS):
        part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, lo:lo + m.SLOTS])), 3)
        for k in LOOP_KEYS + ('eres',):
            np.testing.assert_array_equal(part[k], full[k][:, lo:lo + m.SLOTS], err_msg=k)
    # x_2 = 0.9 (0.9 x_0 + 0.7 u_0) + 0.7 u_1 = 0 at step 0: x_1 of the loop is followed by a u that brings x_2 of that step's plan to 0
    one = run('device', bt)
    assert np.abs(one['X'][0, :, -1, 0]).max() <= PARITY and np.abs(one['U']).max() <= 0.6 + PARITY


# ----------------------------------------------------------------------------- 6. failure isolation
def isolation_batch():
    """box_nu1's model (nx 3, nu 1) at N = 2 from phase 2 (the stages see the phases 2 and 0), three terminal rows: member 1 has Tx = I (N nu = 2 < 3:
    unreachable, status 1), the others one row and two zero rows (reachable); one equality row at phase 0, with a NaN in member 3 (status 3)."""
    c = mq.case_box_nu1()
    nb, p, nx, n = 4, 3, 3, 4
    rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[0], (nb,) + x.shape[1:]))
    Tx = np.zeros((nb, p, 3, nx)); Tx[:, :, :1] = np.random.default_rng(31).standard_normal((1, p, 1, nx))
    Tx[1] = np.eye(3)
    J = np.zeros((nb, p, 1, n)); J[:, :, 0, :] = np.random.default_rng(32).standard_normal((1, p, n))
    J[3, 0, 0, 2] = np.nan
    X0 = 0.2 * np.random.default_rng(33).standard_normal((nb, 2, nx))
    return dict(A=rep(c['A']), B=rep(c['B']), H=rep(c['H']), Pf=rep(c['Pf']), D=rep(c['D']), d=rep(c['d']), q=None, ndcnt=None, J=J, r=None,
                necnt=np.array([[1, 0, 0]] * nb, np.int32), terminal=Tx, X0=X0, N=2, k0=2)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_failing_member_leaves_its_neighbours_bit_identical(entry):
    bt = isolation_batch()
    out = run(entry, bt, max_iter=40)
    print('   status %s iters %s eres %s' % (out['status'].tolist(), out['iters_total'].tolist(), out['eres'].tolist()))
    np.testing.assert_array_equal(out['status'], np.array([[0, 0], [1, 1], [0, 0], [3, 3]]))
    for b in (1, 3):
        for k in ('u0', 'X', 'U', 'lam', 'nu', 'nu_term', 'x1', 'eres', 'hres'):
            assert np.isnan(out[k][b]).all(), k
        assert (out['nact'][b] == -1).all()
    assert (out['iters_total'][1] == 40).all()
    for b in (0, 2):
        alone = run(entry, members(bt, [b]), max_iter=40)
        assert_same({k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in out.items()}, alone, OUT_KEYS + EQ_KEYS)
        assert np.isfinite(out['nu_term'][b]).all() and (out['nu_term'][b, :, 1:] == 0).all() and np.isfinite(out['nu'][b]).all()
        assert (np.abs(out['X'][b, :, -1] @ bt['terminal'][b, (bt['k0'] + bt['N']) % 3, 0]) <= PARITY).all() and (out['eres'][b] == 0).all()


# ----------------------------------------------------------------------------- 7. the edge of the layout
@pytest.mark.parametrize('entry', ENTRIES)
def test_a_row_capacity_that_only_the_layout_with_equality_rows_refuses(entry):
    """(The layout-edge shape itself, nx 40 / nu 24, runs in test 1: case_edge.)"""
    from tunempc_amd import mpc_qp as m
    c = eq.case_edge()
    nd = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    assert m.lds_layout(40, 24, nd, ne=2, nt=3)['bytes'] > m.LDS_BYTES
    D = np.zeros((1, 2, nd, 64)); D[:, :, :4] = c['D']
    d = np.ones((1, 2, nd)); d[:, :, :4] = c['d']
    f = to_dev if entry == 'device' else (lambda x: x)
    args = [f(np.ascontiguousarray(x)) for x in (c['A'], c['B'], c['H'], c['X0'][:, :1])]
    kw = dict(D=f(D), d=f(d), ndcnt=f(np.full((1, 2), 4, np.int32)), Pf=f(c['Pf']))
    plain = to_host(m.mpc_qp_batch(*args, 2, **kw))
    assert not plain['status'].any()
    with pytest.raises(NotImplementedError, match='room for %d rows and 2 equality rows' % nd):
        m.mpc_qp_batch(*args, 2, J=f(c['J']), r=f(c['r']), **kw)


# ----------------------------------------------------------------------------- 8. the reference calling style
def test_the_reference_calling_style_with_rows_and_a_terminal_operator():
    from tunempc_amd import mpc_qp as m
    c = eq.case_rows_mixed_small()
    r = eq.solve_case(c)[0][0]
    p, nx = 3, 3
    A, B, H = [c['A'][0, k] for k in range(p)], [c['B'][0, k] for k in range(p)], c['H'][0]
    Q, R, Nc = [H[k, :nx, :nx] for k in range(p)], [H[k, nx:, nx:] for k in range(p)], [H[k, :nx, nx:] for k in range(p)]
    cnt, ecnt = c['rows'][0], c['erows'][0]
    D = [c['D'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]; d = [c['d'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]
    J = [c['J'][0, k, :ecnt[k]] if ecnt[k] else None for k in range(p)]; rr = [c['r'][0, k, :ecnt[k]] if ecnt[k] else None for k in range(p)]
    kw = dict(D=D, d=d, q=[c['q'][0, k] for k in range(p)], Pf=c['Pf'][0, 0], J=J, r=rr, terminal=[c['Tx'][0, k] for k in range(p)])
    u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, c['X0'][0, 0], c['N'], c['k0'], **kw)
    ms = eq.mult_scale(r)
    assert info['status'] == 0 and relmax(U, r['U']) <= PARITY and relmax(X, r['X']) <= PARITY and np.abs(lam - r['Lam']).max() <= PARITY * ms
    assert np.abs(info['nu'] - r['Nu']).max() <= PARITY * ms and np.abs(info['nu_term'] - r['NuT']).max() <= PARITY * ms and info['eres'] <= PARITY
    log = m.mpc_closed_loop_sim(A, B, Q, R, Nc, c['X0'][0, 0], c['N'], T_LOOP, c['k0'], **kw)
    ref = loop_reference(eq.case_rows_mixed_small)[0][0]
    assert set(log) >= {'x', 'u', 'l', 'h', 'eres'} and len(log['eres']) == T_LOOP and max(log['eres']) <= PARITY
    assert relmax(np.array(log['x']), ref['X']) <= PARITY and relmax(np.array(log['u']), ref['U']) <= PARITY and log['nact'] == ref['nact'].tolist()
    # one matrix for every stage, 'constraint', and an infeasible problem
    args = (np.eye(2) * 0.9, np.array([[0.0], [1.0]]), np.eye(2), np.eye(1), np.zeros((2, 1)), np.array([0.3, -0.2]))
    u0, X, U, lam, info = m.mpc_step(*args, 3, terminal=np.array([[1.0, 1.0]]))
    assert abs(X[-1].sum()) <= PARITY and info['nu_term'].shape == (1,) and info['nu'].shape == (3, 0)
    with pytest.raises(RuntimeError, match='status 1'):
        m.mpc_step(*args, 3, terminal='constraint')                          # B reaches the second state only
    assert 'eres' not in m.mpc_closed_loop_sim(*args, 3, 2)
