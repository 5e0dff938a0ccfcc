"""GPU tests of the affine MPC step and of the loop on a disturbed plant (the AFF instantiations of csrc/tmpc_mpc_qp.h, tunempc_amd.mpc_qp with offset=, qf=,
terminal_rhs=, plant=, disturbance=) against method (b) of tests/mpc_qp_affine_reference.py (the polished solution with its optimality certificate), through the
host and the device entry.

Bounds.  Against the reference: PARITY = 10 x AFF_IPM_VS_POLISH, ten times what the numpy iteration reaches against the same truth (test_mpc_qp_affine_cpu.py,
where it is asserted); u0, X, U relative to max(1, max|.|), lam, nu, nu_term and the slacks relative to max(1, max lam, max|nu|).  The same bound where two
instantiations of the kernel are compared (the shifted cases against the call on the deviation problem, zero arrays against absent ones).  Bit-identity where
the kernel promises it."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_eq_reference as eq  # noqa: E402
import mpc_qp_affine_reference as af  # noqa: E402

PARITY = 10 * af.AFF_IPM_VS_POLISH
ENTRIES = ['host', 'device']
T_LOOP = af.T_LOOP
OUT_KEYS = ('u0', 'X', 'U', 'lam', 'nact', 'hres', 'x1', 'info')
EQ_KEYS = ('nu', 'nu_term', 'eres')
LOOP_KEYS = ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info', 'eres')
ARRAYS = ('D', 'd', 'ndcnt', 'q', 'Pf', 'penalty', 'J', 'r', 'necnt', 'offset', 'qf', 'terminal_rhs', 'disturbance')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def run(entry, bt, steps=None, **kw):
    """mpc_qp_batch (steps None) or mpc_closed_loop_batch on a batch dict of mpc_qp_affine_reference.batch_of (plus plant, disturbance) -> dict of numpy arrays."""
    from tunempc_amd import mpc_qp as m
    f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
    opt = {k: f(bt[k]) for k in ARRAYS if bt.get(k) is not None}
    if bt.get('terminal') is not None:
        opt['terminal'] = bt['terminal'] if isinstance(bt['terminal'], str) else f(bt['terminal'])
    if bt.get('plant') is not None:
        opt['plant'] = tuple(f(x) for x in bt['plant'])
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
    return {k: (tuple(x[idx] for x in v) if k == 'plant' and v is not None else (v[idx] if isinstance(v, np.ndarray) else v)) for k, v in bt.items()}


def keys_of(bt, base):
    return base + (('eps', 'nviol') if bt.get('penalty') is not None else ())


def against(o, r, soft):
    """The outputs of one instance against the dict of solve_aff: every figure relative to its scale."""
    ms = eq.mult_scale(r)
    e = dict(u0=relmax(o['u0'], r['U'][0]), X=relmax(o['X'], r['X']), U=relmax(o['U'], r['U']), lam=np.abs(o['lam'] - r['Lam']).max() / ms if r['Lam'].size else 0.0,
             nu=np.abs(o['nu'] - r['Nu']).max() / ms if r['Nu'].size else 0.0, nu_term=np.abs(o['nu_term'] - r['NuT']).max() / ms if r['NuT'].size else 0.0)
    if soft:
        e['eps'] = np.abs(o['eps'] - r['Eps']).max() / ms
    return e, ms


# ----------------------------------------------------------------------------- 1. the open-loop solution against method (b), and by itself
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', af.VALUE_CASES, ids=[c.__name__ for c in af.VALUE_CASES])
def test_open_loop_solution_against_the_polished_solution(entry, case):
    from tunempc_amd import mpc_qp as m
    c = case()
    ref = af.solve_case(c)
    out = run(entry, af.batch_of(c))
    soft = c['penalty'] is not None
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == 1).all()
    assert (out['iters_total'] <= m.MAX_ITER).all() and (out['pivmin'] > 0).all()
    for b, rb in enumerate(ref):
        kw = af.kwargs(c, b)
        for s, r in enumerate(rb):
            o = {k: out[k][b, s] for k in ('u0', 'X', 'U', 'lam', 'nu', 'nu_term', 'nact', 'eres', 'x1') + (('eps', 'nviol') if soft else ())}
            e, ms = against(o, r, soft)
            k = af.kkt_check_aff(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], o['X'], o['U'], o['lam'], o['nu'], o['nu_term'], o.get('eps'),
                                 None if not soft else c['penalty'][b], **kw)
            print('   %s %s instance %d.%d: iters %d (numpy %d) mu %.1e | vs (b) %s | by itself %s' % (
                entry, c['name'], b, s, out['iters_total'][b, s], r['a']['iters'], out['mu'][b, s], {q: '%.1e' % v for q, v in e.items()}, {q: '%.1e' % v for q, v in k.items()}))
            assert r['b']['certificate'] and r['b']['margin'] >= af.MARGIN_MIN
            assert max(e.values()) <= PARITY, e
            assert o['nact'] == r['nact0'] and (not soft or o['nviol'] == r['nviol0'])
            assert abs(o['eres'] - r['eres0']) <= PARITY and o['eres'] <= PARITY * max(1.0, 0.0 if c['r'] is None else np.abs(c['r']).max())
            assert max(k['dyn'], k['eq'], k['term'], k['comp'], k['comp_e'], k['stat']) <= PARITY and k['viol'] <= PARITY and k['lam_min'] >= -PARITY * ms, k
            assert relmax(o['x1'], r['X'][1]) <= PARITY                          # x1 = A x_0 + B u_0 + c
    nx = c['A'].shape[2]
    assert out['nu'].shape == out['X'].shape[:2] + (c['N'], 0 if c['J'] is None else c['J'].shape[2])
    assert out['nu_term'].shape == out['X'].shape[:2] + (0 if c['Tx'] is None else (nx if isinstance(c['Tx'], str) else c['Tx'].shape[2]),)


# ----------------------------------------------------------------------------- 2. the shifted cases against the call on the deviation problem (the EQ kernels)
@pytest.mark.parametrize('case', af.SHIFT_CASES, ids=[c.__name__ for c in af.SHIFT_CASES])
def test_a_shifted_case_is_the_existing_call_on_the_deviation_problem_plus_the_reference(case):
    """about_reference -> the AFF instantiation; the deviation problem -> the EQ instantiation that served it before.  Each side takes the iteration count
    of the numpy iteration on its own problem."""
    from tunempc_amd import mpc_qp as m
    c = case(); d = c['dev']
    bd = eq.batch_of(d)
    kw = m.about_reference(d['A'], d['B'], d['H'], c['xref'], c['uref'], q=d['q'], Pf=d['Pf'], D=d['D'], d=d['d'], J=d['J'], r=d['r'], terminal=d['Tx'])
    ba = dict(bd, X0=c['X0'], **kw)
    dev = run('device', {k: v for k, v in bd.items()})
    out = run('device', ba)
    assert not dev['status'].any() and not out['status'].any()
    ra, rd = af.solve_case(c), eq.solve_case(d)
    soft = c['penalty'] is not None
    for b in range(c['X0'].shape[0]):
        for s in range(c['X0'].shape[1]):
            Xs, Us = af.shifted_solution(c, dict(X=dev['X'][b, s], U=dev['U'][b, s]), b)
            ms = eq.mult_scale(rd[b][s])
            e = dict(X=relmax(out['X'][b, s], Xs), U=relmax(out['U'][b, s], Us), u0=relmax(out['u0'][b, s], Us[0]),
                     **{k: np.abs(out[k][b, s] - dev[k][b, s]).max() / ms for k in ('lam', 'nu', 'nu_term') + (('eps',) if soft else ()) if dev[k][b, s].size})
            print('   %s instance %d.%d: iters %d (numpy %d), deviation problem %d (numpy %d) | %s' % (
                c['name'], b, s, out['iters_total'][b, s], ra[b][s]['a']['iters'], dev['iters_total'][b, s], rd[b][s]['a']['iters'], {q: '%.1e' % v for q, v in e.items()}))
            assert max(e.values()) <= PARITY, e
            assert out['nact'][b, s] == dev['nact'][b, s] and (not soft or out['nviol'][b, s] == dev['nviol'][b, s])
            assert out['iters_total'][b, s] == ra[b][s]['a']['iters'] and dev['iters_total'][b, s] == rd[b][s]['a']['iters']


# ----------------------------------------------------------------------------- 3. no rows at all: the affine LQ problem
@pytest.mark.parametrize('entry', ENTRIES)
def test_without_rows_the_step_is_the_affine_lq_problem(entry):
    c = af.case_aff_no_rows()
    kw = af.kwargs(c)
    out = run(entry, af.batch_of(c))
    assert not out['status'].any() and out['lam'].shape[-1] == 0 and out['nu'].shape[-1] == 0 and out['nu_term'].shape[-1] == 0
    assert (out['nact'] == 0).all() and np.isneginf(out['hres']).all() and (out['eres'] == 0).all()
    for s in range(c['X0'].shape[1]):
        X, U = af.lq_condensed(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], q=kw['q'], Pf=kw['Pf'], offset=kw['offset'], qf=kw['qf'])
        e = dict(X=relmax(out['X'][0, s], X), U=relmax(out['U'][0, s], U), x1=relmax(out['x1'][0, s], X[1]))
        print('   %s instance %d: iters %d | against the dense solve %s' % (entry, s, out['iters_total'][0, s], {q: '%.1e' % v for q, v in e.items()}))
        assert max(e.values()) <= PARITY, e


# ----------------------------------------------------------------------------- 4. the loops over T = 7
@functools.lru_cache(maxsize=None)
def loop_reference(which):
    if which == 'shift':
        c = af.loop_shift()
        return [af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], x0, T_LOOP, **af.kwargs(c)) for x0 in c['X0'][0]]
    c, plant, W = af.loop_plant()
    return [af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], x0, T_LOOP, plant=(plant[0][0], plant[1][0]), W=W[0, s], **af.kwargs(c))
            for s, x0 in enumerate(c['X0'][0])]


def loop_against(entry, name, out, ref):
    for s, r in enumerate(ref):
        assert r['status'] == 0 and r['certificate'] and r['margin'] >= af.MARGIN_MIN, (s, r['margin'])
        fin = np.isfinite(r['hres'])
        e = dict(X=relmax(out['X'][0, s], r['X']), U=relmax(out['U'][0, s], r['U']), hres=relmax(out['hres'][0, s][fin], r['hres'][fin]),
                 eres=np.abs(out['eres'][0, s] - r['eres']).max())
        print('   %s %s instance %d: iters %s nact %s | %s' % (entry, name, s, out['iters'][0, s].tolist(), out['nact'][0, s].tolist(), {q: '%.1e' % v for q, v in e.items()}))
        assert max(e.values()) <= PARITY, e
        np.testing.assert_array_equal(out['nact'][0, s], r['nact'])


@pytest.mark.parametrize('entry', ENTRIES)
def test_the_loop_in_absolute_coordinates_is_the_deviation_loop_plus_the_reference(entry):
    c = af.loop_shift(); d = c['dev']
    out = run(entry, af.batch_of(c), T_LOOP)
    assert not out['status'].any() and (out['steps'] == T_LOOP).all()
    loop_against(entry, '(i)', out, loop_reference('shift'))
    dev = run(entry, eq.batch_of(d), T_LOOP)
    ph = (c['k0'] + np.arange(T_LOOP + 1)) % c['A'].shape[1]
    e = max(relmax(out['X'][0], dev['X'][0] + c['xref'][0][ph]), relmax(out['U'][0], dev['U'][0] + c['uref'][0][ph[:T_LOOP]]))
    print('   %s (i): against the GPU loop on the deviation problem plus the reference %.1e' % (entry, e))
    assert not dev['status'].any() and e <= PARITY
    np.testing.assert_array_equal(out['nact'], dev['nact'])
    one = run(entry, af.batch_of(c))
    np.testing.assert_array_equal(one['u0'], out['u0']); np.testing.assert_array_equal(one['x1'], out['X'][:, :, 1])


@pytest.mark.parametrize('entry', ENTRIES)
def test_the_loop_on_a_plant_that_is_not_the_model(entry):
    c, plant, W = af.loop_plant()
    bt = dict(af.batch_of(c), plant=plant, disturbance=W)
    out = run(entry, bt, T_LOOP)
    assert not out['status'].any() and (out['steps'] == T_LOOP).all()
    loop_against(entry, '(ii)', out, loop_reference('plant'))
    model = run(entry, af.batch_of(c), T_LOOP)
    assert np.abs(out['X'] - model['X']).max() > 1e-2
    np.testing.assert_array_equal(out['u0'], model['u0'])                    # the controller does not know about the plant
    short = run(entry, bt, T_LOOP, return_traj=False)
    assert short['X'] is None and short['U'] is None
    assert_same(short, out, [k for k in LOOP_KEYS if k not in ('X', 'U')])


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_disturbance_across_a_hard_bound_ends_the_loop_and_a_soft_bound_carries_it(entry):
    """(iii), the point of the plant arguments: the state that the soft rows exist for is now produced by the loop itself."""
    c, W, ts = af.loop_push()
    bt = dict(af.batch_of(c), disturbance=W)
    hard = run(entry, bt, T_LOOP)
    soft = run(entry, dict(bt, penalty=np.full(c['d'].shape, af.PUSH_PENALTY)), T_LOOP)
    kw = af.kwargs(c)
    ref = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, 0], T_LOOP, penalty=np.full(c['d'].shape[1:], af.PUSH_PENALTY), W=W[0, 0], **kw)
    print('   %s (iii) t* %d: hard status %d after %d steps; soft status %d, x_1 %s, nviol %s, iters %s' % (
        entry, ts, hard['status'][0, 0], hard['steps'][0, 0], soft['status'][0, 0], np.round(soft['X'][0, 0, :, 0], 4).tolist(), soft['nviol'][0, 0].tolist(),
        soft['iters'][0, 0].tolist()))
    assert hard['status'][0, 0] == 1 and hard['steps'][0, 0] == ts
    assert np.isfinite(hard['X'][0, 0, :ts + 1]).all() and np.isnan(hard['X'][0, 0, ts + 1:]).all() and abs(hard['X'][0, 0, ts, 0]) > 2 * af.X1_BOUND
    assert (np.abs(hard['X'][0, 0, :ts, 0]) < af.X1_BOUND).all() and (hard['nact'][0, 0, ts:] == -1).all()
    assert soft['status'][0, 0] == 0 and soft['steps'][0, 0] == T_LOOP and soft['nviol'][0, 0, ts] >= 1 and soft['hres'][0, 0, ts] > af.X1_BOUND
    assert (np.abs(soft['X'][0, 0, ts + 1:, 0]) <= af.X1_BOUND + PARITY).all()
    assert ref['status'] == 0 and relmax(soft['X'][0, 0], ref['X']) <= PARITY and relmax(soft['U'][0, 0], ref['U']) <= PARITY
    assert relmax(hard['X'][0, 0, :ts + 1], soft['X'][0, 0, :ts + 1]) <= PARITY                          # no row is active before the push


# ----------------------------------------------------------------------------- 5. bit-identity
@pytest.mark.parametrize('case', [mq.case_mixed_small, mq.case_box_bench], ids=['mixed_small', 'box_bench'])
def test_without_the_affine_arguments_the_call_is_the_existing_one_bit_for_bit(case):
    """None through the keywords, and seven NULL pointers through the new C entries, against the calls without them: hard, soft and eq."""
    from tunempc_amd import _lib
    c = case()
    bt = dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=c['rows'].astype(np.int32), N=c['N'], k0=c['k0'])
    pen = np.full(c['d'].shape, 0.3)
    for entry in ENTRIES:
        f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
        for penalty, terminal in ((None, None), (pen, None), (None, 'constraint'), (pen, 'constraint')):
            b2 = dict(bt, penalty=penalty, terminal=terminal)
            plain = run(entry, b2, T_LOOP); kw = run(entry, dict(b2, offset=None, qf=None, terminal_rhs=None, plant=None, disturbance=None), T_LOOP)
            keys = tuple(k for k in keys_of(b2, LOOP_KEYS if terminal else LOOP_KEYS[:-1]) if k != 'eps')
            assert_same(plain, kw, keys)
            assert ('eres' in kw) == (terminal is not None)
            a = [f(b2[k]) for k in ('A', 'B', 'H', 'q', 'Pf', 'D', 'ndcnt', 'd')]
            fa = _lib.mpc_qp_aff_batch_device if entry == 'device' else _lib.mpc_qp_aff_batch_host
            fe = _lib.mpc_qp_eq_batch_device if entry == 'device' else _lib.mpc_qp_eq_batch_host
            new = to_host(fa(*a, f(penalty), None, None, None, terminal, (None,) * 7, f(b2['X0']), c['N'], T_LOOP, c['k0'], 1e-10, 60, True, False))
            old = to_host(fe(*a, f(penalty), None, None, None, terminal, f(b2['X0']), c['N'], T_LOOP, c['k0'], 1e-10, 60, True, False))
            assert_same(new, old, ('U0', 'XT', 'info', 'X', 'U', 'iters', 'nact', 'hres', 'eres') + (('nviol',) if penalty is not None else ()))
            np.testing.assert_array_equal(new['X'], plain['X'])


@pytest.mark.parametrize('case', [eq.case_rows_mixed_small, eq.case_soft, eq.case_term_box_bench], ids=['rows_mixed_small', 'soft', 'term_box_bench'])
def test_zero_arrays_and_the_model_as_the_plant_change_nothing_beyond_rounding(case):
    """All seven pointers given against the same call without them: another instantiation of the kernel, so the bound is PARITY and not the bits."""
    c = case()
    bt = eq.batch_of(c)
    nb, p, nx, _ = c['A'].shape
    ns = c['X0'].shape[1]
    nt = nx if isinstance(c['Tx'], str) else c['Tx'].shape[2]
    z = np.zeros
    full = dict(bt, offset=z((nb, p, nx)), qf=z((nb, p, nx)), terminal_rhs=z((nb, p, nt)), plant=(c['A'], c['B'], z((nb, p, nx))), disturbance=z((nb, ns, T_LOOP, nx)))
    for entry in ENTRIES:
        a, b = run(entry, full, T_LOOP), run(entry, bt, T_LOOP)
        fin = np.isfinite(b['hres'])
        np.testing.assert_array_equal(np.isfinite(a['hres']), fin)
        e = dict(X=relmax(a['X'], b['X']), U=relmax(a['U'], b['U']), hres=relmax(a['hres'][fin], b['hres'][fin]), eres=np.abs(a['eres'] - b['eres']).max())
        print('   %s %s: %s, iters equal %s' % (entry, c['name'], {q: '%.1e' % v for q, v in e.items()}, bool((a['iters'] == b['iters']).all())))
        assert not a['status'].any() and max(e.values()) <= PARITY
        np.testing.assert_array_equal(a['nact'], b['nact'])


@pytest.mark.parametrize('case', [af.case_shift_rows_mixed_small, af.case_aff_tx_soft_box_nu2, af.case_aff_bench, af.case_aff_no_rows],
                         ids=['shift_rows_mixed_small', 'aff_tx_soft_box_nu2', 'aff_bench', 'aff_no_rows'])
def test_entries_neighbours_and_absent_outputs_do_not_change_a_bit(case):
    c = case()
    nb, ns, nx = c['X0'].shape
    rng = np.random.default_rng(81)
    bt = dict(af.batch_of(c), plant=(c['A'] + 0.02 * rng.standard_normal(c['A'].shape), c['B'], 0.01 * rng.standard_normal((nb, c['A'].shape[1], nx))),
              disturbance=0.01 * rng.standard_normal((nb, ns, T_LOOP, nx)))
    keys = tuple(k for k in keys_of(bt, LOOP_KEYS) if k != 'eps')
    dev = run('device', bt, T_LOOP); host = run('host', bt, T_LOOP)
    assert not dev['status'].any()
    assert_same(dev, host, keys)
    one = {k: v for k, v in bt.items() if k not in ('plant', 'disturbance')}
    assert_same(run('device', one), run('host', one), keys_of(bt, OUT_KEYS + EQ_KEYS))
    for s in range(min(ns, 3)):
        for width in (1, 2, 3):
            part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, s:s + width]), disturbance=np.ascontiguousarray(bt['disturbance'][:, s:s + width])), T_LOOP)
            for k in keys:
                np.testing.assert_array_equal(part[k][:, 0], dev[k][:, s], err_msg='%s of state %d in a call of %d' % (k, s, width))
    full = run('device', one); short = run('device', one, return_traj=False)
    assert short['X'] is None and short['U'] is None and short['lam'] is None and short['nu'] is None and short['nu_term'] is None
    assert_same(short, full, [k for k in keys_of(bt, OUT_KEYS + ('eres',)) if k not in ('X', 'U', 'lam', 'eps')])


def test_more_instances_than_workspace_slots():
    """nx = nu = 1, N = 2, the box |u| <= 0.6, x_2 = 0.1, the offset 0.05 and a disturbance per instance: 549 instances on 512 slots."""
    from tunempc_amd import mpc_qp as m
    ns = m.SLOTS + 37
    D = np.array([[[[0.0, 1.0], [0.0, -1.0]]]])
    bt = dict(A=np.array([[[[0.9]]]]), B=np.array([[[[0.7]]]]), H=np.array([[[[2.0, 0.3], [0.3, 1.5]]]]), Pf=np.array([[[[1.2]]]]), D=D, d=np.full((1, 1, 2), 0.6),
              X0=np.linspace(-0.8, 0.8, ns).reshape(1, -1, 1), N=2, k0=0, q=None, ndcnt=None, terminal='constraint', terminal_rhs=np.array([[[0.1]]]),
              offset=np.array([[[0.05]]]), disturbance=0.05 * np.random.default_rng(82).standard_normal((1, ns, 3, 1)))
    full = run('device', bt, 3)
    assert not full['status'].any() and (full['nact'][0, :, 0] == 1).any() and (full['nact'][0, :, 0] == 0).any()
    for lo in range(0, ns, m.SLOTS):
        part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, lo:lo + m.SLOTS]), disturbance=np.ascontiguousarray(bt['disturbance'][:, lo:lo + m.SLOTS])), 3)
        for k in LOOP_KEYS:
            np.testing.assert_array_equal(part[k], full[k][:, lo:lo + m.SLOTS], err_msg=k)
    one = run('device', {k: v for k, v in bt.items() if k != 'disturbance'})
    assert np.abs(one['X'][0, :, -1, 0] - 0.1).max() <= PARITY and np.abs(one['U']).max() <= 0.6 + PARITY
    np.testing.assert_allclose(full['X'][0, :, 1, 0], one['x1'][0, :, 0] + bt['disturbance'][0, :, 0, 0], rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------- 6. failure isolation
T_ISO = 6


def isolation_batch():
    """box_nu1's model (nx 3, nu 1, p 3) at N = 2 from phase 2, one terminal row with t != 0, an offset, a disturbance, T = 6.  Step t sees the phases
    (2 + t) % 3, (3 + t) % 3 in its dynamics and k_N = (4 + t) % 3.  Member 1: NaN in offset at phase 1, first met at step 1.  Member 3: NaN in terminal_rhs
    at phase 0, first met at step 2.  Member 4: NaN in W at step 3 of its second state: x_4 is not finite and step 4 ends.  Members 0 and 2 are sound."""
    c = mq.case_box_nu1()
    nb, p, nx, ns = 5, 3, 3, 2
    rep = lambda x: np.ascontiguousarray(np.broadcast_to(x[0], (nb,) + x.shape[1:]))
    Tx = np.ascontiguousarray(np.broadcast_to(np.random.default_rng(31).standard_normal((1, p, 1, nx)), (nb, p, 1, nx)))
    off = 0.05 * np.random.default_rng(91).standard_normal((nb, p, nx)); off[1, 1, 2] = np.nan
    trh = 0.05 * np.random.default_rng(92).standard_normal((nb, p, 1)); trh[3, 0, 0] = np.nan
    W = 0.02 * np.random.default_rng(93).standard_normal((nb, ns, T_ISO, nx)); W[4, 1, 3, 0] = np.nan
    X0 = 0.2 * np.random.default_rng(33).standard_normal((nb, ns, nx))
    return dict(A=rep(c['A']), B=rep(c['B']), H=rep(c['H']), Pf=rep(c['Pf']), D=rep(c['D']), d=rep(c['d']), q=None, ndcnt=None, terminal=Tx, terminal_rhs=trh,
                offset=off, disturbance=W, X0=X0, N=2, k0=2)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_non_finite_entry_ends_its_instance_at_the_step_that_meets_it(entry):
    bt = isolation_batch()
    out = run(entry, bt, T_ISO)
    print('   status %s steps %s' % (out['status'].tolist(), out['steps'].tolist()))
    np.testing.assert_array_equal(out['status'], np.array([[0, 0], [3, 3], [0, 0], [3, 3], [0, 3]]))
    np.testing.assert_array_equal(out['steps'], np.array([[6, 6], [1, 1], [6, 6], [2, 2], [6, 4]]))
    for b, s, t in ((1, 0, 1), (1, 1, 1), (3, 0, 2), (3, 1, 2), (4, 1, 4)):
        keep = t + 1 if b != 4 else t                                        # (x_4 of member 4 holds the NaN of W_3 in its first entry)
        assert np.isfinite(out['X'][b, s, :keep]).all() and np.isfinite(out['U'][b, s, :t]).all()
        assert np.isnan(out['X'][b, s, t + 1:]).all() and np.isnan(out['U'][b, s, t:]).all() and np.isnan(out['XT'][b, s]).all()
        assert (out['nact'][b, s, t:] == -1).all() and (out['nact'][b, s, :t] >= 0).all() and np.isnan(out['eres'][b, s, t:]).all()
    assert np.isnan(out['X'][4, 1, 4, 0]) and np.isfinite(out['X'][4, 1, 4, 1:]).all()
    for b in (0, 2):
        alone = run(entry, members(bt, [b]), T_ISO)
        assert_same({k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in out.items()}, alone, LOOP_KEYS)
    alone = run(entry, dict(members(bt, [4]), X0=np.ascontiguousarray(bt['X0'][4:5, :1]), disturbance=np.ascontiguousarray(bt['disturbance'][4:5, :1])), T_ISO)
    for k in LOOP_KEYS:
        np.testing.assert_array_equal(alone[k][:, 0], out[k][4:5, 0], err_msg=k)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_terminal_right_hand_side_out_of_reach_is_status_1(entry):
    i = af.infeasible_instance()
    out = run(entry, dict(i, q=None))
    print('   status %d after %d iterations, r_p %.1e' % (out['status'][0, 0], out['iters_total'][0, 0], out['rp'][0, 0]))
    assert out['status'][0, 0] == 1 and out['iters_total'][0, 0] == 60 and np.isnan(out['u0']).all() and out['rp'][0, 0] > 1e-3
    ok = run(entry, dict(i, q=None, N=5))                                    # the same target within reach of five inputs
    assert ok['status'][0, 0] == 0 and np.abs(ok['X'][0, 0, -1] - i['terminal_rhs'][0, (2 + 5) % 3]).max() <= PARITY


# ----------------------------------------------------------------------------- 7. the reference calling style
def test_the_reference_calling_style_in_absolute_coordinates():
    from tunempc_amd import mpc_qp as m
    c = af.case_shift_rows_mixed_small()
    r = af.solve_case(c)[0][0]
    p, nx = 3, 3
    A, B, H = [c['A'][0, k] for k in range(p)], [c['B'][0, k] for k in range(p)], c['H'][0]
    Q, R, Nc = [H[k, :nx, :nx] for k in range(p)], [H[k, nx:, nx:] for k in range(p)], [H[k, :nx, nx:] for k in range(p)]
    cnt, ecnt = c['rows'][0], c['erows'][0]
    D = [c['D'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]; d = [c['d'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]
    J = [c['J'][0, k, :ecnt[k]] if ecnt[k] else None for k in range(p)]; rr = [c['r'][0, k, :ecnt[k]] if ecnt[k] else None for k in range(p)]
    kw = dict(D=D, d=d, q=[c['q'][0, k] for k in range(p)], Pf=c['Pf'][0, 0], J=J, r=rr, terminal=[c['Tx'][0, k] for k in range(p)],
              offset=[c['offset'][0, k] for k in range(p)], qf=[c['qf'][0, k] for k in range(p)], terminal_rhs=[c['trhs'][0, k] for k in range(p)])
    u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, c['X0'][0, 0], c['N'], c['k0'], **kw)
    ms = eq.mult_scale(r)
    assert info['status'] == 0 and relmax(U, r['U']) <= PARITY and relmax(X, r['X']) <= PARITY and np.abs(lam - r['Lam']).max() <= PARITY * ms
    assert np.abs(info['nu'] - r['Nu']).max() <= PARITY * ms and np.abs(info['nu_term'] - r['NuT']).max() <= PARITY * ms
    rng = np.random.default_rng(83)
    Ap = [a + 0.02 * rng.standard_normal(a.shape) for a in A]
    W = 0.01 * rng.standard_normal((T_LOOP, nx))
    log = m.mpc_closed_loop_sim(A, B, Q, R, Nc, c['X0'][0, 0], c['N'], T_LOOP, c['k0'], plant=(Ap, B), disturbance=W, **kw)
    ref = af.closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, 0], T_LOOP, plant=(np.array(Ap), c['B'][0]), W=W, **af.kwargs(c))
    assert ref['status'] == 0 and ref['certificate'] and ref['margin'] >= af.MARGIN_MIN
    assert set(log) >= {'x', 'u', 'l', 'h', 'eres'} and len(log['x']) == T_LOOP + 1
    assert relmax(np.array(log['x']), ref['X']) <= PARITY and relmax(np.array(log['u']), ref['U']) <= PARITY and log['nact'] == ref['nact'].tolist()
    # one vector for every stage: x+ = 0.9 x + [0; 1] u + c, x_3 on the line x_1 + x_2 = 0.2
    args = (np.eye(2) * 0.9, np.array([[0.0], [1.0]]), np.eye(2), np.eye(1), np.zeros((2, 1)), np.array([0.3, -0.2]))
    u0, X, U, lam, info = m.mpc_step(*args, 3, terminal=np.array([[1.0, 1.0]]), terminal_rhs=np.array([0.2]), offset=np.array([0.01, -0.02]))
    assert abs(X[-1].sum() - 0.2) <= PARITY and np.abs(X[1] - (0.9 * X[0] + np.array([0.0, U[0, 0]]) + np.array([0.01, -0.02]))).max() <= PARITY
    with pytest.raises(RuntimeError, match='status 1'):
        m.mpc_step(*args, 3, terminal='constraint', terminal_rhs=np.array([0.5, 0.0]))         # B reaches the second state only
