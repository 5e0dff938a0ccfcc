"""GPU tests of the MPC step with quadratic slack penalties (the QUAD instantiations of csrc/tmpc_mpc_qp.h, tunempc_amd.mpc_qp with penalty2=) against method
(b) of tests/mpc_qp_quad_reference.py (the polished solution with its optimality certificate), through the host and the device entry.

Bounds.  Against the reference: PARITY = 10 x QUAD_IPM_VS_POLISH, ten times what the numpy iteration reaches against the same truth (test_mpc_qp_quad_cpu.py,
where it is asserted); u0, X, U relative to max(1, max|.|), lam relative to max(1, max lam), the slacks relative to max(1, max e).  Bit-identity where the
kernel promises it: penalty2 all zeros against the call with penalty only, the two entries, an instance alone against the same instance among others, absent
optional outputs, more instances than workspace slots.  Iteration counts are printed, not compared."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_horizon_reference as lh  # noqa: E402
import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_soft_reference as sq  # noqa: E402
import mpc_qp_eq_reference as eqr  # noqa: E402
import mpc_qp_affine_reference as af  # noqa: E402
import mpc_qp_quad_reference as qq  # noqa: E402

PARITY = 10 * qq.QUAD_IPM_VS_POLISH
ENTRIES = ['host', 'device']
T_LOOP = 7
OUT_KEYS = ('u0', 'X', 'U', 'lam', 'nact', 'hres', 'x1', 'info')
LOOP_KEYS = ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def run(entry, bt, steps=None, penalty='own', penalty2='own', **kw):
    """mpc_qp_batch (steps None) or mpc_closed_loop_batch on a batch dict (A, B, H, X0, q, Pf, D, d, ndcnt, penalty, penalty2, N, k0) -> dict of numpy arrays.
    penalty, penalty2: 'own' the batch's, None without, or an array.  kw: further keywords, arrays moved to the device for that entry."""
    from tunempc_amd import mpc_qp as m
    f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
    opt = {k: f(bt[k]) for k in ('D', 'd', 'ndcnt', 'q', 'Pf') if bt.get(k) is not None}
    for nm, v in (('penalty', penalty), ('penalty2', penalty2)):
        v = bt.get(nm) if isinstance(v, str) else v
        if v is not None:
            opt[nm] = f(v)
    kw = {k: (f(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
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


# ----------------------------------------------------------------------------- 1. the analytic case: every size is one, rows +-x <= b on the state
def scalar_batch(x0s, c, Z, N=2):
    """x+ = a x + u, cost 1/2 (x^2 + r u^2) per stage, rows +-x <= b.  With N = 2 only x_1 is free under the rows (x_0 is given, x_2 carries no row)."""
    a, r, b = 0.9, 0.5, 0.3
    bt = dict(A=np.array([[[[a]]]]), B=np.array([[[[1.0]]]]), H=np.array([[[[1.0, 0.0], [0.0, r]]]]), Pf=None, D=np.array([[[[1.0, 0.0], [-1.0, 0.0]]]]),
              d=np.full((1, 1, 2), b), penalty=np.full((1, 1, 2), c), penalty2=np.full((1, 1, 2), Z), X0=np.asarray(x0s, float).reshape(1, -1, 1), N=N, k0=0,
              q=None, ndcnt=None)
    return bt, a, r, b


def scalar_truth(x0, a, r, b, c, Z):
    """N = 2: u_1 = 0, so the cost in y = x_1 is 1/2 (1 + r) y^2 - r a x0 y + penalty(e), e = max(0, |y| - b) -> y, e, lam of the binding row (x0 >= 0)."""
    g = 1.0 + r
    y = r * a * x0 / g
    if y <= b:
        return y, 0.0, 0.0
    lam_b = r * a * x0 - g * b                                               # the multiplier that holds y on the bound
    if lam_b <= c:
        return b, 0.0, lam_b
    e = (lam_b - c) / (g + Z)                                                # g (b + e) - r a x0 + c + Z e = 0
    return b + e, e, c + Z * e


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('c,Z', [(0.0, 4.0), (0.6, 4.0)], ids=['pure', 'l1+l2'])
def test_the_scalar_step_with_a_quadratic_penalty_in_closed_form(entry, c, Z):
    x0s = (0.5, 1.6, 4.0) if c > 0 else (0.5, 4.0)                           # free, (L1 + L2 only: held on the bound,) violated
    bt, a, r, b = scalar_batch(x0s, c, Z)
    out = run(entry, bt)
    kinds = []
    for s, x0 in enumerate(x0s):
        y, e, lam = scalar_truth(x0, a, r, b, c, Z)
        kinds.append((e > 0, lam > 0))
        print('   x0 %+.1f: x1 %+.12f (want %+.12f) eps %.3e (want %.3e) lam %.6f (want %.6f) iters %d nact %d nviol %d' % (
            x0, out['X'][0, s, 1, 0], y, out['eps'][0, s, 1, 0], e, out['lam'][0, s, 1, 0], lam, out['iters_total'][0, s], out['nact'][0, s], out['nviol'][0, s]))
        assert out['status'][0, s] == 0 and abs(out['X'][0, s, 1, 0] - y) <= PARITY * max(1.0, abs(y)) and abs(out['u0'][0, s, 0] - (y - a * x0)) <= PARITY * max(1.0, abs(x0))
        assert abs(out['eps'][0, s, 1, 0] - e) <= PARITY * max(1.0, e) and abs(out['lam'][0, s, 1, 0] - lam) <= PARITY * max(1.0, lam)
        assert (np.abs(out['eps'][0, s, 1, 1]) <= PARITY) and abs(out['lam'][0, s, 1, 1]) <= PARITY           # the opposite row
    assert kinds == ([(False, False), (False, True), (True, True)] if c > 0 else [(False, False), (True, True)])
    # stage 0 acts on x_0 alone: x_0 = 0.5 > b violates it whatever u does; its slack is x_0 - b and hres is that slack
    assert abs(out['hres'][0, 0] - (0.5 - b)) <= 1e-15 and abs(out['eps'][0, 0, 0, 0] - (0.5 - b)) <= PARITY and out['nviol'][0, 0] == 1 and out['nact'][0, 0] == 1
    assert out['eps'].shape == (1, len(x0s), 2, 2) and out['nviol'].dtype == np.int32


# ----------------------------------------------------------------------------- 2. the open-loop solution against method (b), and by itself
def gpu_states(o, cvec2, zvec2):
    """The pattern of a returned solution: cvec2, zvec2 [N, nd] the weights of every row."""
    pure = (cvec2 == 0) & (zvec2 > 0)
    vio = (o['eps'] > qq.MARGIN_MIN / 2) & ~pure
    act = (o['lam'] > qq.MARGIN_MIN / 2) & ~vio
    return np.where(vio, qq.VIOLATED, np.where(act, qq.ACTIVE, qq.INACTIVE))


def stage_weights(i):
    p = i['penalty'].shape[0]
    return (np.stack([i['penalty'][(i['k0'] + j) % p] for j in range(i['N'])]), np.stack([i['penalty2'][(i['k0'] + j) % p] for j in range(i['N'])]))


def check_open_loop(tag, o, i, r, iters, mu):
    lmax = max(1.0, np.abs(r['Lam']).max()); emax = max(1.0, np.abs(r['Eps']).max())
    e = dict(u0=relmax(o['u0'], r['U'][0]), X=relmax(o['X'], r['X']), U=relmax(o['U'], r['U']), lam=np.abs(o['lam'] - r['Lam']).max() / lmax,
             eps=np.abs(o['eps'] - r['Eps']).max() / emax)
    k = qq.kkt_check_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], o['X'], o['U'], o['lam'], o['eps'], i['penalty'], i['penalty2'], **i['kw'])
    print('   %s: iters %d (numpy %d) mu %.1e | vs (b) %s | by itself %s' % (tag, iters, r['a']['iters'], mu, {q: '%.1e' % v for q, v in e.items()},
                                                                        {q: '%.1e' % v for q, v in k.items()}))
    assert r['b']['certificate'] and r['b']['margin'] >= qq.MARGIN_MIN
    assert max(e.values()) <= PARITY, e
    assert o['nact'] == r['nact0'] and o['nviol'] == r['nviol0']
    cw, zw = stage_weights(i)
    rows = np.arange(cw.shape[1])[None] < np.array([i['kw']['rows'][(i['k0'] + j) % len(i['kw']['rows'])] for j in range(i['N'])])[:, None]
    np.testing.assert_array_equal(np.where(rows, gpu_states(o, cw, zw), 0), r['State'])
    assert max(k['dyn'], k['viol'], k['comp'], k['comp_e'], k['stat'], k['quad_v'], k['pure']) <= PARITY and k['low'] >= -PARITY * lmax, k
    assert (o['eps'][~np.isfinite(cw)] == 0).all() and (o['eps'] >= 0).all()


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('kind,case,f,zeta,hard_first', qq.VARIANTS, ids=qq.VARIANT_IDS)
def test_open_loop_solution_against_the_polished_solution(entry, kind, case, f, zeta, hard_first):
    from tunempc_amd import mpc_qp as m
    insts = qq.instances(kind, case, f, zeta, hard_first)
    ref = qq.solve_instances(kind, case, f, zeta, hard_first)
    out = run(entry, qq.batch_of(insts))
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == 1).all()
    assert (out['iters_total'] <= m.MAX_ITER).all() and (out['pivmin'] > 0).all()
    for b, (i, r) in enumerate(zip(insts, ref)):
        o = {k: out[k][b, 0] for k in ('u0', 'X', 'U', 'lam', 'eps', 'nact', 'nviol')}
        check_open_loop('%s instance %d' % (entry, b), o, i, r, out['iters_total'][b, 0], out['mu'][b, 0])


# ----------------------------------------------------------------------------- 3. the lifted problem through the existing hard entry
@pytest.mark.parametrize('kind,case,f,zeta', [v[:4] for v in qq.VARIANTS if v[1] in qq.SMALL and not v[4]],
                         ids=[i for i, v in zip(qq.VARIANT_IDS, qq.VARIANTS) if v[1] in qq.SMALL and not v[4]])
def test_the_lifted_problem_through_the_hard_entry_agrees(kind, case, f, zeta):
    insts = qq.instances(kind, case, f, zeta)
    ref = qq.solve_instances(kind, case, f, zeta)
    lifted = []
    for i in insts:
        L = qq.lift_quad(i['A'], i['B'], i['H'], i['penalty'], i['penalty2'], q=i['kw']['q'], D=i['kw']['D'], d=i['kw']['d'], rows=i['kw']['rows'])
        lifted.append(dict(A=L['A'], B=L['B'], H=L['H'], N=i['N'], k0=i['k0'], x0=i['x0'], penalty=i['penalty'],
                           kw=dict(q=L['q'], Pf=i['kw']['Pf'], D=L['D'], d=L['d'], rows=L['rows'])))
    lift = run('device', sq.batch_of(lifted), penalty=None, penalty2=None)
    quad = run('device', qq.batch_of(insts))
    mb = insts[0]['B'].shape[2]
    assert not lift['status'].any() and not quad['status'].any() and 'eps' not in lift
    for b, r in enumerate(ref):
        e = dict(u0=relmax(lift['u0'][b, 0, :mb], r['U'][0]), X=relmax(lift['X'][b, 0], r['X']), U=relmax(lift['U'][b, 0, :, :mb], r['U']),
                 eps=np.abs(lift['U'][b, 0, :, mb:] - r['Eps']).max() / max(1.0, np.abs(r['Eps']).max()))
        g = dict(u0=relmax(lift['u0'][b, 0, :mb], quad['u0'][b, 0]), X=relmax(lift['X'][b, 0], quad['X'][b, 0]), U=relmax(lift['U'][b, 0, :, :mb], quad['U'][b, 0]))
        print('   instance %d: iters lifted %d eliminated %d | lifted vs (b) %s | lifted vs eliminated %s' % (
            b, lift['iters_total'][b, 0], quad['iters_total'][b, 0], {q: '%.1e' % v for q, v in e.items()}, {q: '%.1e' % v for q, v in g.items()}))
        assert max(e.values()) <= PARITY and max(g.values()) <= 2 * PARITY, (e, g)


# ----------------------------------------------------------------------------- 4. the closed loop over T = 7 against the loop on method (b)
LOOPS = [('l12', mq.case_box_nu1, 0.3, 1.0), ('l12', mq.case_mixed_small, 0.3, 100.0), ('pure', mq.case_box_nu2, 1e2, 0.0), ('pure', mq.case_mixed_small, 1e3, 0.0),
         ('l12', mq.case_box_bench, 0.3, 1.0), ('pure', mq.case_box_bench, 1e2, 0.0)]
LOOP_IDS = ['%s-%s-f%g' % (k, c.__name__, f) for k, c, f, z in LOOPS]


@functools.lru_cache(maxsize=None)
def loop_reference(kind, case, f, zeta):
    return [qq.closed_loop_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], T_LOOP, i['penalty'], i['penalty2'], **i['kw'])
            for i in qq.instances(kind, case, f, zeta)]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('kind,case,f,zeta', LOOPS, ids=LOOP_IDS)
def test_closed_loop_against_the_loop_on_the_polished_solution(entry, kind, case, f, zeta):
    ref = loop_reference(kind, case, f, zeta)
    bt = qq.batch_of(qq.instances(kind, case, f, zeta))
    out = run(entry, bt, T_LOOP)
    nb = len(ref)
    assert out['nviol'].shape == (nb, 1, T_LOOP) and not out['status'].any() and (out['steps'] == T_LOOP).all()
    for b, r in enumerate(ref):
        assert r['certificate'] and r['margin'] >= qq.MARGIN_MIN, (b, r['margin'])
        fin = np.isfinite(r['hres'])
        e = dict(X=relmax(out['X'][b, 0], r['X']), U=relmax(out['U'][b, 0], r['U']), hres=relmax(out['hres'][b, 0][fin], r['hres'][fin]))
        print('   %s instance %d: iters %s nact %s nviol %s | %s' % (entry, b, out['iters'][b, 0].tolist(), out['nact'][b, 0].tolist(), out['nviol'][b, 0].tolist(),
                                                                {q: '%.1e' % v for q, v in e.items()}))
        assert max(e.values()) <= PARITY, e
        np.testing.assert_array_equal(out['nact'][b, 0], r['nact']); np.testing.assert_array_equal(out['nviol'][b, 0], r['nviol'])
        np.testing.assert_array_equal(np.isneginf(out['hres'][b, 0]), ~fin)
    assert out['nviol'].sum() >= 1 and (out['hres'] > 0).any()
    one = run(entry, bt)
    np.testing.assert_array_equal(one['u0'], out['u0']); np.testing.assert_array_equal(one['nviol'], out['nviol'][:, :, 0])
    short = run(entry, bt, T_LOOP, return_traj=False)
    assert short['X'] is None and short['U'] is None
    assert_same(short, out, [k for k in LOOP_KEYS + ('nviol',) if k not in ('X', 'U')])


def infeasible_batch(c, Z):
    """Member 0: x_0 outside the bound with (c, Z) on its rows.  Member 1: the same model with hard rows (penalty inf, Z = 0) and x_0 inside them."""
    cs = sq.case_infeasible_when_hard()
    two = lambda x: None if x is None else np.ascontiguousarray(np.concatenate([x, x]))
    return dict(A=two(cs['A']), B=two(cs['B']), H=two(cs['H']), Pf=two(cs['Pf']), D=two(cs['D']), d=two(cs['d']), q=None, ndcnt=None, N=cs['N'], k0=cs['k0'],
                X0=np.array([[[1.0, 0.2, -0.3]], [[0.05, 0.2, -0.3]]]), penalty=np.concatenate([np.full_like(cs['penalty'], c), np.full_like(cs['penalty'], np.inf)]),
                penalty2=np.concatenate([np.full_like(cs['penalty'], Z), np.zeros_like(cs['penalty'])]))


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('c,Z', qq.INFEASIBLE, ids=['c%g-Z%g' % cz for cz in qq.INFEASIBLE])
def test_a_start_outside_a_bound_is_solved_and_a_hard_neighbour_is_untouched(entry, c, Z):
    """Status 1 when hard, status 0 with the quadratic penalty; hres is the slack at step 0.  After step 0 the rows of stage 0 act on x_0 alone and sit on or near
    their bound, so nact / nviol of those steps are compared only where the reference's margin tells them apart."""
    bt = infeasible_batch(c, Z)
    i = qq.infeasible_instance(c, Z)
    hard = run(entry, bt, penalty=None, penalty2=None)
    assert hard['status'][0, 0] == 1 and np.isnan(hard['u0'][0]).all() and hard['nact'][0, 0] == -1
    r = qq.solve_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], i['penalty2'], **i['kw'])
    out = run(entry, bt)
    print('   status %s iters %s hres %s nviol %s eps of stage 0 %s' % (out['status'][:, 0].tolist(), out['iters_total'][:, 0].tolist(), out['hres'][:, 0].tolist(),
                                                                 out['nviol'][:, 0].tolist(), out['eps'][0, 0, 0].tolist()))
    assert not out['status'].any()
    o = {k: out[k][0, 0] for k in ('u0', 'X', 'U', 'lam', 'eps', 'nact', 'nviol')}
    check_open_loop('%s infeasible start' % entry, o, i, r, out['iters_total'][0, 0], out['mu'][0, 0])
    assert abs(out['hres'][0, 0] - 0.9) <= 1e-15 and abs(out['hres'][0, 0] - out['eps'][0, 0, 0].max()) <= PARITY and out['nviol'][0, 0] == 1
    # the loop: hres equals the slack at step 0
    ref = qq.closed_loop_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], T_LOOP, i['penalty'], i['penalty2'], **i['kw'])
    loop = run(entry, bt, T_LOOP)
    e = dict(X=relmax(loop['X'][0, 0], ref['X']), U=relmax(loop['U'][0, 0], ref['U']), hres=relmax(loop['hres'][0, 0], ref['hres']))
    print('   loop: iters %s hres %s | %s' % (loop['iters'][0, 0].tolist(), loop['hres'][0, 0].tolist(), e))
    assert not loop['status'].any() and ref['certificate'] and max(e.values()) <= PARITY, e
    assert abs(loop['hres'][0, 0, 0] - ref['usc'][0]) <= PARITY and loop['nviol'][0, 0, 0] == 1
    # the hard neighbour: the same bits as alone, with the quad kernel and without penalties
    assert out['hres'][1, 0] <= PARITY and out['nviol'][1, 0] == 0 and (out['eps'][1] == 0).all()
    alone = run(entry, members(bt, [1]))
    assert_same({k: v[1:] for k, v in out.items()}, alone, OUT_KEYS + ('eps', 'nviol'))
    assert_same({k: v[1:] for k, v in hard.items()}, alone, OUT_KEYS)
    assert_same({k: v[1:] for k, v in loop.items()}, run(entry, members(bt, [1]), T_LOOP), LOOP_KEYS + ('nviol',))


# ----------------------------------------------------------------------------- 5. bit-identity
def shared_batch(kind, case, f, zeta):
    """A case as it is (ns states per problem) with one pair of weights per problem: that of its first instance."""
    c = case()
    nb = c['A'].shape[0]
    ins = qq.instances(kind, case, f, zeta)
    per = len(ins) // nb
    return dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=c['rows'].astype(np.int32), N=c['N'], k0=c['k0'],
                penalty=np.stack([ins[b * per]['penalty'] for b in range(nb)]), penalty2=np.stack([ins[b * per]['penalty2'] for b in range(nb)]))


@pytest.mark.parametrize('case,hard_first', [(mq.case_mixed_small, False), (mq.case_box_bench, True)], ids=['mixed_small', 'box_bench-mixed'])
def test_a_penalty2_of_zeros_is_the_soft_call_bit_for_bit(case, hard_first):
    bt = shared_batch('l12', case, 0.3, 1.0)
    if hard_first:
        bt['penalty'][:, :, 0] = np.inf                                      # a hard row among them
    zero = np.zeros_like(bt['penalty2'])
    for entry in ENTRIES:
        soft, quad0 = run(entry, bt, penalty2=None), run(entry, bt, penalty2=zero)
        assert not soft['status'].any() and (soft['eps'] > qq.MARGIN_MIN).any() and 'eres' not in soft and not quad0['eres'].any()
        assert_same(soft, quad0, OUT_KEYS + ('eps', 'nviol'))
        softT, quadT = run(entry, bt, T_LOOP, penalty2=None), run(entry, bt, T_LOOP, penalty2=zero)
        assert_same(softT, quadT, LOOP_KEYS + ('nviol',))
        # ... and with terminal='constraint' the soft EQ kernel against the QUAD AFF kernel
        assert_same(run(entry, bt, penalty2=None, terminal='constraint'), run(entry, bt, penalty2=zero, terminal='constraint'),
                    OUT_KEYS + ('eps', 'nviol', 'nu', 'nu_term', 'eres'))


@pytest.mark.parametrize('kind,case,f,zeta,hard_first', [('l12', mq.case_mixed_small, 0.3, 100.0, True), ('pure', mq.case_box_bench, 1e2, 0.0, False)],
                         ids=['l12-mixed_small-mixed', 'pure-box_bench'])
def test_entries_neighbours_and_absent_outputs_do_not_change_a_bit(kind, case, f, zeta, hard_first):
    bt = shared_batch(kind, case, f, zeta)
    if hard_first:
        bt['penalty'][:, :, 0] = np.inf; bt['penalty2'][:, :, 0] = 0.0
    keys = LOOP_KEYS + ('nviol',)
    dev = run('device', bt, T_LOOP); host = run('host', bt, T_LOOP)
    assert not dev['status'].any() and dev['nviol'].sum() >= 1
    assert_same(dev, host, keys)
    assert_same(run('device', bt), run('host', bt), OUT_KEYS + ('eps', 'nviol'))
    ns = bt['X0'].shape[1]
    for s in range(min(ns, 2)):
        for width in (1, 2, 3):
            part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, s:s + width])), T_LOOP)
            for k in keys:
                np.testing.assert_array_equal(part[k][:, 0], dev[k][:, s], err_msg='%s of state %d in a call of %d' % (k, s, width))
    full = run('device', bt); short = run('device', bt, return_traj=False)
    assert short['X'] is None and short['U'] is None and short['lam'] is None and short['eps'] is None
    assert_same(short, full, [k for k in OUT_KEYS + ('nviol',) if k not in ('X', 'U', 'lam')])


def test_more_instances_than_workspace_slots():
    from tunempc_amd import mpc_qp as m
    ns = m.SLOTS + 37
    x0s = np.linspace(0.0, 5.0, ns)
    bt, a, r, b = scalar_batch(x0s, 0.0, 4.0)
    full = run('device', bt, 3)
    assert not full['status'].any() and (full['nviol'][0, :, 0] == 1).any() and (full['nviol'][0, :, 0] == 0).any()
    for lo in range(0, ns, m.SLOTS):
        part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, lo:lo + m.SLOTS])), 3)
        for k in LOOP_KEYS + ('nviol',):
            np.testing.assert_array_equal(part[k], full[k][:, lo:lo + m.SLOTS], err_msg=k)
    want = np.array([scalar_truth(x, a, r, b, 0.0, 4.0)[0] for x in x0s])
    np.testing.assert_allclose(full['X'][0, :, 1, 0], want, rtol=0, atol=PARITY * max(1.0, np.abs(want).max()))


# ----------------------------------------------------------------------------- 6. composition with the equality rows and the affine problem
def lifted_eq_kw(i, extra):
    """The lifted problem of an instance (the slacks as inputs) with the keywords of the EQ / affine reference: J gets zero columns for the slacks."""
    L = qq.lift_quad(i['A'], i['B'], i['H'], i['penalty'], i['penalty2'], q=i['kw']['q'], D=i['kw']['D'], d=i['kw']['d'], rows=i['kw']['rows'])
    kw = dict(q=L['q'], Pf=i['kw']['Pf'], D=L['D'], d=L['d'], rows=L['rows'], **{k: v for k, v in extra.items() if k != 'J'})
    if 'J' in extra:
        J = extra['J']
        kw['J'] = np.concatenate([J, np.zeros(J.shape[:2] + (L['B'].shape[2] - i['B'].shape[2],))], axis=2)
    return L, kw


def compose_instance(kind):
    i = qq.instances(kind, mq.case_mixed_small, 0.3 if kind == 'l12' else 1e2, 100.0 if kind == 'l12' else 0.0)[1]
    return i, i['B'].shape[2]


def batch1(i):
    return qq.batch_of([i])


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('kind', ['l12', 'pure'])
def test_quadratic_rows_with_equality_rows_and_the_terminal_constraint(entry, kind):
    i, mb = compose_instance(kind)
    p, n = i['A'].shape[0], i['A'].shape[1] + mb
    J = np.random.default_rng(3).standard_normal((p, 1, n)); rr = 0.05 * np.ones((p, 1))
    L, kw = lifted_eq_kw(i, dict(J=J, r=rr, Tx='constraint'))
    r = eqr.solve_eq(L['A'], L['B'], L['H'], i['N'], i['k0'], i['x0'], **kw)
    assert r['a']['status'] == 0 and r['b']['certificate'] and r['b']['margin'] >= qq.MARGIN_MIN, r['b']['margin']
    out = run(entry, batch1(i), J=J[None], r=rr[None], terminal='constraint')
    eps = r['U'][:, mb:]
    e = dict(X=relmax(out['X'][0, 0], r['X']), U=relmax(out['U'][0, 0], r['U'][:, :mb]), eps=np.abs(out['eps'][0, 0] - eps).max() / max(1.0, eps.max()),
             nu=np.abs(out['nu'][0, 0] - r['Nu']).max() / eqr.mult_scale(r), xN=np.abs(out['X'][0, 0, -1]).max(), eres=out['eres'][0, 0])
    print('   %s %s: iters %d | %s, slacks > 0: %d' % (entry, kind, out['iters_total'][0, 0], {q: '%.1e' % v for q, v in e.items()}, int((eps > qq.MARGIN_MIN).sum())))
    assert out['status'][0, 0] == 0 and max(e.values()) <= PARITY, e
    assert (eps > qq.MARGIN_MIN).any()


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('kind', ['l12', 'pure'])
def test_quadratic_rows_with_an_offset_and_a_disturbed_loop(entry, kind):
    i, mb = compose_instance(kind)
    p, nx = i['A'].shape[0], i['A'].shape[1]
    rng = np.random.default_rng(4)
    off = 0.1 * rng.standard_normal((p, nx)); W = 0.05 * rng.standard_normal((T_LOOP, nx))
    L, kw = lifted_eq_kw(i, dict(offset=off))
    r = af.solve_aff(L['A'], L['B'], L['H'], i['N'], i['k0'], i['x0'], **kw)
    assert r['a']['status'] == 0 and r['b']['certificate'] and r['b']['margin'] >= qq.MARGIN_MIN, r['b']['margin']
    out = run(entry, batch1(i), offset=off[None])
    eps = r['U'][:, mb:]
    e = dict(X=relmax(out['X'][0, 0], r['X']), U=relmax(out['U'][0, 0], r['U'][:, :mb]), eps=np.abs(out['eps'][0, 0] - eps).max() / max(1.0, eps.max()))
    print('   %s %s offset: iters %d | %s' % (entry, kind, out['iters_total'][0, 0], {q: '%.1e' % v for q, v in e.items()}))
    assert out['status'][0, 0] == 0 and max(e.values()) <= PARITY, e
    cl = af.closed_loop_aff(L['A'], L['B'], L['H'], i['N'], i['k0'], i['x0'], T_LOOP, W=W, **kw)
    assert cl['status'] == 0 and cl['certificate'] and cl['margin'] >= qq.MARGIN_MIN, cl['margin']
    loop = run(entry, batch1(i), T_LOOP, offset=off[None], disturbance=W[None, None])
    e = dict(X=relmax(loop['X'][0, 0], cl['X']), U=relmax(loop['U'][0, 0], cl['U'][:, :mb]))
    print('   %s %s disturbed loop: iters %s nviol %s | %s' % (entry, kind, loop['iters'][0, 0].tolist(), loop['nviol'][0, 0].tolist(), {q: '%.1e' % v for q, v in e.items()}))
    assert loop['status'][0, 0] == 0 and max(e.values()) <= PARITY, e


# ----------------------------------------------------------------------------- 7. failure isolation
@pytest.mark.parametrize('what', ['nan', 'negative', 'on_hard', 'both_zero'])
def test_an_invalid_penalty2_ends_that_member_and_leaves_the_others_alone(what):
    """Rows: +-u_1 <= 0.2 hard, u_2 <= 0.05 with (c, Z).  Member 1 carries the invalid pair (device entry: status 3 before step 0; Python and the host entry
    refuse it); members 0 and 2 are sound."""
    from tunempc_amd import _lib
    base = lh.case_ragged_rows()
    nb, p, nx, mb, n = 3, 3, 3, 2, 5
    A = np.ascontiguousarray(np.broadcast_to(base['A'][0], (nb, p, nx, nx))); B = np.ascontiguousarray(np.broadcast_to(base['B'][0], (nb, p, nx, mb)))
    H = np.ascontiguousarray(np.broadcast_to(base['Hc'][0], (nb, p, n, n)))
    D = np.zeros((nb, p, 3, n)); D[:, :, 0, nx] = 1.0; D[:, :, 1, nx] = -1.0; D[:, :, 2, nx + 1] = 1.0
    d = np.full((nb, p, 3), 0.2); d[:, :, 2] = 0.05
    pen = np.full((nb, p, 3), np.inf); pen[:, :, 2] = 0.05
    pen2 = np.zeros((nb, p, 3)); pen2[:, :, 2] = 2.0
    pen[2, :, 2] = 0.0                                                       # member 2: pure quadratic
    if what == 'nan':
        pen2[1, 1, 2] = np.nan
    elif what == 'negative':
        pen2[1, 1, 2] = -1.0
    elif what == 'on_hard':
        pen2[1, 2, 0] = 1.0
    else:
        pen[1, 0, 2] = 0.0; pen2[1, 0, 2] = 0.0
    X0 = np.random.default_rng(8).standard_normal((nb, 2, nx))
    T = 4

    def call(idx):
        dv = [to_dev(x[idx]) for x in (A, B, H, D, d, pen, pen2, X0)]
        return to_host(_lib.mpc_qp_quad_batch_device(dv[0], dv[1], dv[2], None, None, dv[3], None, dv[4], dv[5], None, None, None, None, None, dv[6], dv[7], 1, T, 0,
                                                     1e-10, 40, True, False))
    out = call(slice(None))
    st = out['info'][..., 0].astype(int); steps = out['info'][..., 1].astype(int)
    print('   status %s steps %s iters %s nviol %s' % (st.tolist(), steps.tolist(), out['iters'][:, 0].tolist(), out['nviol'][:, 0].tolist()))
    np.testing.assert_array_equal(st, np.array([[0, 0], [3, 3], [0, 0]]))
    np.testing.assert_array_equal(steps, np.array([[T, T], [0, 0], [T, T]]))
    assert np.isnan(out['X'][1, :, 1:]).all() and np.isnan(out['U'][1]).all() and np.isnan(out['XT'][1]).all() and np.isnan(out['hres'][1]).all()
    assert (out['nact'][1] == -1).all() and (out['nviol'][1] == -1).all() and np.isnan(out['U0'][1]).all()
    assert out['nviol'][[0, 2]].sum() >= 1
    sound = call([0, 2])
    for k in ('X', 'U', 'iters', 'nact', 'nviol', 'hres', 'XT', 'U0', 'info'):
        np.testing.assert_array_equal(sound[k], out[k][[0, 2]], err_msg=k)
    with pytest.raises(ValueError, match='penalty2?\\[1\\]\\[%d\\]\\[%d\\] = ' % {'nan': (1, 2), 'negative': (1, 2), 'on_hard': (2, 0), 'both_zero': (0, 2)}[what]):
        _lib.mpc_qp_quad_batch_host(A, B, H, None, None, D, None, d, pen, None, None, None, None, None, pen2, X0, 1, T, 0, 1e-10, 40, True, False)


# ----------------------------------------------------------------------------- 8. the reference calling style
def test_the_reference_calling_style_with_penalty2():
    from tunempc_amd import mpc_qp as m
    c = mq.case_mixed_small()
    p, nx = 3, 3
    cnt = c['rows'][0]
    for kind, f, zeta in (('l12', 0.3, 100.0), ('pure', 1e2, 0.0)):
        i = qq.instances(kind, mq.case_mixed_small, f, zeta)[0]
        r = qq.solve_instances(kind, mq.case_mixed_small, f, zeta)[0]
        A, B, H = [i['A'][k] for k in range(p)], [i['B'][k] for k in range(p)], i['H']
        Q, R, Nc = [H[k, :nx, :nx] for k in range(p)], [H[k, nx:, nx:] for k in range(p)], [H[k, :nx, nx:] for k in range(p)]
        D = [c['D'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]; d = [c['d'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]
        pen = [i['penalty'][k, :cnt[k]] if cnt[k] else None for k in range(p)]; pen2 = [i['penalty2'][k, :cnt[k]] if cnt[k] else None for k in range(p)]
        kw = dict(D=D, d=d, q=[c['q'][0, k] for k in range(p)], Pf=c['Pf'][0, 0], penalty2=pen2)
        if kind == 'l12':
            kw['penalty'] = pen                                              # (pure: penalty left out, the rows with Z > 0 are pure quadratic)
        u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, i['x0'], c['N'], c['k0'], **kw)
        lmax = max(1.0, r['Lam'].max()); emax = max(1.0, r['Eps'].max())
        assert info['status'] == 0 and relmax(U, r['U']) <= PARITY and relmax(X, r['X']) <= PARITY and np.abs(lam - r['Lam']).max() <= PARITY * lmax
        assert np.abs(info['eps'] - r['Eps']).max() <= PARITY * emax and info['nviol'] == r['nviol0'] and r['b']['nviol'] >= 1
        log = m.mpc_closed_loop_sim(A, B, Q, R, Nc, i['x0'], c['N'], T_LOOP, c['k0'], **kw)
        ref = loop_reference(kind, mq.case_mixed_small, f, zeta)[0]
        assert set(log) >= {'x', 'u', 'l', 'h', 'usc', 'nviol'} and len(log['usc']) == len(log['h']) == T_LOOP
        assert relmax(np.array(log['x']), ref['X']) <= PARITY and relmax(np.array(log['u']), ref['U']) <= PARITY
        assert log['nact'] == ref['nact'].tolist() and log['nviol'] == ref['nviol'].tolist() and sum(log['nviol']) >= 1
        for t in range(T_LOOP):
            m_t = cnt[(c['k0'] + t) % p]
            assert log['usc'][t].shape == (m_t,) and (log['usc'][t] >= 0).all()
            if m_t:
                assert abs(log['usc'][t].max() - max(0.0, ref['hres'][t])) <= PARITY and abs(log['usc'][t].max() - ref['usc'][t]) <= PARITY
    # one vector for every stage: rows +-x <= 0.1 on a scalar model, L1 + L2 on the first and hard on the second; then pure quadratic on the first
    one = dict(D=np.array([[0.0, 1.0], [0.0, -1.0]]), d=np.array([0.1, 0.1]))
    args = (np.eye(1) * 0.9, np.ones((1, 1)), np.eye(1), np.eye(1), np.zeros((1, 1)), -np.ones(1) * 3.0, 2)
    u0, X, U, lam, info = m.mpc_step(*args, penalty=np.array([0.5, np.inf]), penalty2=np.array([2.0, 0.0]), **one)
    assert info['nviol'] == 1 and info['eps'][0, 0] > 0 and (info['eps'][:, 1] == 0).all() and abs(lam[0, 0] - 0.5 - 2.0 * info['eps'][0, 0]) <= PARITY
    u0, X, U, lam, info = m.mpc_step(*args, penalty2=np.array([2.0, 0.0]), **one)
    assert info['nviol'] == 1 and info['eps'][0, 0] > 0 and (info['eps'][:, 1] == 0).all() and abs(lam[0, 0] - 2.0 * info['eps'][0, 0]) <= PARITY
    log = m.mpc_closed_loop_sim(*args, 3, penalty2=[np.array([2.0, 0.0])], **one)
    assert 'usc' in log and log['usc'][0][0] > 0 and log['usc'][0][1] == 0 and 'usc' not in m.mpc_closed_loop_sim(*args, 3, **one)
