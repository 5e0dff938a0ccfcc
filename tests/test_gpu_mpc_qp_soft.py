"""GPU tests of the MPC step with soft rows (the SOFT instantiation of csrc/tmpc_mpc_qp.h, tunempc_amd.mpc_qp with penalty=) against method (b) of
tests/mpc_qp_soft_reference.py (the polished three-state solution with its optimality certificate), through the host and the device entry.

Bounds.  Against the reference: PARITY = 10 x SOFT_IPM_VS_POLISH = 3e-8, ten times what the numpy eliminated iteration reaches against the same truth
(test_mpc_qp_soft_cpu.py, where it is asserted); u0, X, U relative to max(1, max|.|), lam and the slacks relative to max(1, max lam).  Bit-identity where the
kernel promises it: penalty None or all inf against the call without penalty, the two entries, an instance alone against the same instance among others, absent
optional outputs, more instances than workspace slots.  Iteration counts are printed, not compared."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_horizon_reference as lh  # noqa: E402
import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_soft_reference as sq  # noqa: E402

PARITY = 10 * sq.SOFT_IPM_VS_POLISH
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


def run(entry, bt, steps=None, penalty='own', **kw):
    """mpc_qp_batch (steps None) or mpc_closed_loop_batch on a batch dict (A, B, H, X0, q, Pf, D, d, ndcnt, penalty, N, k0) -> dict of numpy arrays.
    penalty: 'own' the batch's, None without, or an array."""
    from tunempc_amd import mpc_qp as m
    f = to_dev if entry == 'device' else (lambda x: None if x is None else np.ascontiguousarray(x))
    opt = {k: f(bt[k]) for k in ('D', 'd', 'ndcnt', 'q', 'Pf') if bt.get(k) is not None}
    pen = bt['penalty'] if isinstance(penalty, str) else penalty
    if pen is not None:
        opt['penalty'] = f(pen)
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


# ----------------------------------------------------------------------------- 1. the analytic case: every size is one
def scalar_batch(x0s, c=3.0):
    a, b, umax = 0.9, 0.7, 0.25
    S = 1.5 + b * b * 1.2
    K = (0.3 + b * 1.2 * a) / S
    bt = dict(A=np.array([[[[a]]]]), B=np.array([[[[b]]]]), H=np.array([[[[2.0, 0.3], [0.3, 1.5]]]]), Pf=np.array([[[[1.2]]]]), D=np.array([[[[0.0, 1.0]]]]),
              d=np.full((1, 1, 1), umax), penalty=np.full((1, 1, 1), c), X0=np.asarray(x0s, float).reshape(1, -1, 1), N=1, k0=0, q=None, ndcnt=None)
    return bt, K, S, umax


def scalar_truth(x0, K, S, umax, c):
    """f'(u) = S (u + K x): free, exactly penalised (lam = -f'(umax) < c) or violated (f'(u) = -c) -> u, e, lam."""
    u = -K * x0
    if u <= umax:
        return u, 0.0, 0.0
    lam = -S * (umax + K * x0)
    if lam < c:
        return umax, 0.0, lam
    u = -K * x0 - c / S
    return u, u - umax, c


@pytest.mark.parametrize('entry', ENTRIES)
def test_the_scalar_soft_step_in_closed_form(entry):
    c = 3.0
    x0s = (0.2, -2.0, -5.0)                                                  # free, exactly penalised, violated
    bt, K, S, umax = scalar_batch(x0s, c)
    out = run(entry, bt)
    kinds = []
    for s, x0 in enumerate(x0s):
        u, e, lam = scalar_truth(x0, K, S, umax, c)
        kinds.append((e > 0, lam > 0))
        print('   x0 %+.1f: u0 %+.12f (want %+.12f) eps %.3e (want %.3e) lam %.6f (want %.6f) iters %d nact %d nviol %d' % (
            x0, out['u0'][0, s, 0], u, out['eps'][0, s, 0, 0], e, out['lam'][0, s, 0, 0], lam, out['iters_total'][0, s], out['nact'][0, s], out['nviol'][0, s]))
        assert out['status'][0, s] == 0 and abs(out['u0'][0, s, 0] - u) <= PARITY * max(1.0, abs(u))
        assert abs(out['eps'][0, s, 0, 0] - e) <= PARITY * max(1.0, c) and abs(out['lam'][0, s, 0, 0] - lam) <= PARITY * max(1.0, c)
        assert out['nact'][0, s] == (1 if lam > 0 else 0) and out['nviol'][0, s] == (1 if e > 0 else 0)
        assert abs(out['hres'][0, s] - (u - umax)) <= PARITY and abs(out['x1'][0, s, 0] - (0.9 * x0 + 0.7 * out['u0'][0, s, 0])) <= 1e-15
    assert kinds == [(False, False), (False, True), (True, True)]
    assert out['eps'].shape == (1, 3, 1, 1) and out['nviol'].dtype == np.int32


# ----------------------------------------------------------------------------- 2. the open-loop solution against method (b), and by itself
def gpu_states(out_b, lam_scale):
    vio = out_b['eps'] > sq.MARGIN_MIN / 2
    act = (out_b['lam'] > sq.MARGIN_MIN / 2) & ~vio
    return np.where(vio, sq.VIOLATED, np.where(act, sq.ACTIVE, sq.INACTIVE))


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case,f,hard_first', sq.VARIANTS, ids=sq.VARIANT_IDS)
def test_open_loop_solution_against_the_polished_three_state_solution(entry, case, f, hard_first):
    from tunempc_amd import mpc_qp as m
    insts = sq.instances(case, f, hard_first)
    ref = sq.solve_instances(case, f, hard_first)
    out = run(entry, sq.batch_of(insts))
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == 1).all()
    assert (out['iters_total'] <= m.MAX_ITER).all() and (out['pivmin'] > 0).all()
    for b, (i, r) in enumerate(zip(insts, ref)):
        o = {k: out[k][b, 0] for k in ('u0', 'X', 'U', 'lam', 'eps', 'nact', 'nviol')}
        lmax = max(1.0, np.abs(r['Lam']).max())
        e = dict(u0=relmax(o['u0'], r['U'][0]), X=relmax(o['X'], r['X']), U=relmax(o['U'], r['U']), lam=np.abs(o['lam'] - r['Lam']).max() / lmax,
                 eps=np.abs(o['eps'] - r['Eps']).max() / lmax)
        k = sq.kkt_check_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], o['X'], o['U'], o['lam'], o['eps'], i['penalty'], **i['kw'])
        print('   %s instance %d: iters %d (numpy %d) mu %.1e | vs (b) %s | by itself %s' % (entry, b, out['iters_total'][b, 0], r['a']['iters'], out['mu'][b, 0],
                                                                                       {q: '%.1e' % v for q, v in e.items()}, {q: '%.1e' % v for q, v in k.items()}))
        assert r['b']['certificate'] and r['b']['margin'] >= sq.MARGIN_MIN
        assert max(e.values()) <= PARITY, e
        assert o['nact'] == r['nact0'] and o['nviol'] == r['nviol0']
        np.testing.assert_array_equal(gpu_states(o, lmax), r['State'])
        assert max(k['dyn'], k['viol'], k['comp'], k['comp_e'], k['stat']) <= PARITY and k['low'] >= -PARITY * lmax, k
        hard = ~np.isfinite(np.stack([i['penalty'][(i['k0'] + j) % i['penalty'].shape[0]] for j in range(i['N'])]))
        assert (o['eps'][hard] == 0).all() and (o['eps'] >= 0).all()


# ----------------------------------------------------------------------------- 3. the exact penalty
@pytest.mark.parametrize('case', sq.CASES, ids=[c.__name__ for c in sq.CASES])
@pytest.mark.parametrize('f', [10.0, 1e3])
def test_the_exact_penalty_gives_the_hard_solution(case, f):
    bt = sq.batch_of(sq.instances(case, f))
    soft, hard = run('device', bt), run('device', bt, penalty=None)
    assert not soft['status'].any() and not hard['status'].any() and 'eps' not in hard
    lmax = max(1.0, np.abs(hard['lam']).max())
    e = dict(u0=relmax(soft['u0'], hard['u0']), X=relmax(soft['X'], hard['X']), U=relmax(soft['U'], hard['U']), lam=np.abs(soft['lam'] - hard['lam']).max() / lmax,
             eps=soft['eps'].max() / lmax)
    print('   iters soft %s hard %s | %s' % (soft['iters_total'][:, 0].tolist(), hard['iters_total'][:, 0].tolist(), {q: '%.1e' % v for q, v in e.items()}))
    assert max(e.values()) <= PARITY, e
    assert (soft['nviol'] == 0).all() and (soft['nact'] == hard['nact']).all() and (soft['hres'] <= PARITY).all()


# ----------------------------------------------------------------------------- 4. infeasible when hard
def infeasible_batch():
    """Member 0: x_0 outside the soft bound.  Member 1: the same model with hard rows (penalty inf) and x_0 inside them."""
    c = sq.case_infeasible_when_hard()
    two = lambda x: None if x is None else np.ascontiguousarray(np.concatenate([x, x]))
    bt = dict(A=two(c['A']), B=two(c['B']), H=two(c['H']), Pf=two(c['Pf']), D=two(c['D']), d=two(c['d']), q=None, ndcnt=None, N=c['N'], k0=c['k0'],
              X0=np.array([[[1.0, 0.2, -0.3]], [[0.05, 0.2, -0.3]]]), penalty=np.concatenate([c['penalty'], np.full_like(c['penalty'], np.inf)]))
    return bt


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_start_outside_a_soft_bound_is_solved_and_a_hard_neighbour_is_untouched(entry):
    bt = infeasible_batch()
    i = sq.infeasible_instance()
    r = sq.solve_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], **i['kw'])
    hard = run(entry, bt, penalty=None)
    assert hard['status'][0, 0] == 1 and np.isnan(hard['u0'][0]).all() and np.isnan(hard['X'][0]).all() and hard['nact'][0, 0] == -1
    out = run(entry, bt)
    print('   status %s iters %s hres %s nviol %s eps of stage 0 %s' % (out['status'][:, 0].tolist(), out['iters_total'][:, 0].tolist(), out['hres'][:, 0].tolist(),
                                                                 out['nviol'][:, 0].tolist(), out['eps'][0, 0, 0].tolist()))
    assert not out['status'].any()
    assert out['hres'][0, 0] > 0 and abs(out['hres'][0, 0] - out['eps'][0, 0, 0].max()) <= PARITY and abs(out['hres'][0, 0] - 0.9) <= PARITY and out['nviol'][0, 0] >= 1
    lmax = max(1.0, r['Lam'].max())
    assert relmax(out['U'][0, 0], r['U']) <= PARITY and relmax(out['X'][0, 0], r['X']) <= PARITY and np.abs(out['lam'][0, 0] - r['Lam']).max() <= PARITY * lmax
    assert np.abs(out['eps'][0, 0] - r['Eps']).max() <= PARITY * lmax and out['nviol'][0, 0] == r['nviol0']
    # the hard neighbour: the same bits as alone, with all-inf penalties and without penalty
    assert out['hres'][1, 0] <= PARITY and out['nviol'][1, 0] == 0 and (out['eps'][1] == 0).all()
    alone = run(entry, members(bt, [1]))
    assert_same({k: v[1:] for k, v in out.items()}, alone, OUT_KEYS + ('eps', 'nviol'))
    assert_same({k: v[1:] for k, v in hard.items()}, alone, OUT_KEYS)


# ----------------------------------------------------------------------------- 5. the closed loop over T = 7 against the loop on method (b)
LOOP_CASES = sq.SMALL + [mq.case_box_bench]


@functools.lru_cache(maxsize=None)
def loop_reference(case, f):
    return [sq.closed_loop_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], T_LOOP, i['penalty'], **i['kw']) for i in sq.instances(case, f)]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', LOOP_CASES, ids=[c.__name__ for c in LOOP_CASES])
@pytest.mark.parametrize('f', [0.3, 10.0])
def test_closed_loop_against_the_loop_on_the_polished_solution(entry, case, f):
    ref = loop_reference(case, f)
    bt = sq.batch_of(sq.instances(case, f))
    out = run(entry, bt, T_LOOP)
    nb = len(ref)
    assert out['nviol'].shape == (nb, 1, T_LOOP) and not out['status'].any() and (out['steps'] == T_LOOP).all()
    for b, r in enumerate(ref):
        assert r['certificate'] and r['margin'] >= sq.MARGIN_MIN, (b, r['margin'])
        fin = np.isfinite(r['hres'])
        e = dict(X=relmax(out['X'][b, 0], r['X']), U=relmax(out['U'][b, 0], r['U']), hres=relmax(out['hres'][b, 0][fin], r['hres'][fin]))
        print('   %s instance %d: iters %s nact %s nviol %s | %s' % (entry, b, out['iters'][b, 0].tolist(), out['nact'][b, 0].tolist(), out['nviol'][b, 0].tolist(),
                                                                {q: '%.1e' % v for q, v in e.items()}))
        assert max(e.values()) <= PARITY, e
        np.testing.assert_array_equal(out['nact'][b, 0], r['nact']); np.testing.assert_array_equal(out['nviol'][b, 0], r['nviol'])
        np.testing.assert_array_equal(np.isneginf(out['hres'][b, 0]), ~fin)
    if f < 1:
        assert out['nviol'].sum() >= 1 and (out['hres'] > sq.MARGIN_MIN).any()
    one = run(entry, bt)
    np.testing.assert_array_equal(one['u0'], out['u0']); np.testing.assert_array_equal(one['nviol'], out['nviol'][:, :, 0])
    short = run(entry, bt, T_LOOP, return_traj=False)
    assert short['X'] is None and short['U'] is None
    assert_same(short, out, [k for k in LOOP_KEYS + ('nviol',) if k not in ('X', 'U')])


@pytest.mark.parametrize('entry', ENTRIES)
def test_the_violation_of_an_infeasible_start_is_gone_after_one_step(entry):
    """The reference loop (test_mpc_qp_soft_cpu.py): hres = 0.9 at step 0, then x stays on the bound and |hres| is rounding.  The rows of stage 0 act on x_0 alone
    there and sit exactly on their bound, so nact / nviol of those steps are not defined by the problem and are not compared."""
    i = sq.infeasible_instance()
    ref = sq.closed_loop_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], T_LOOP, i['penalty'], **i['kw'])
    out = run(entry, members(infeasible_batch(), [0]), T_LOOP)
    e = dict(X=relmax(out['X'][0, 0], ref['X']), U=relmax(out['U'][0, 0], ref['U']), hres=relmax(out['hres'][0, 0], ref['hres']))
    print('   iters %s hres %s | %s' % (out['iters'][0, 0].tolist(), out['hres'][0, 0].tolist(), e))
    assert out['status'][0, 0] == 0 and max(e.values()) <= PARITY, e
    assert out['hres'][0, 0, 0] > 0.5 and out['nviol'][0, 0, 0] == 1 and (np.abs(out['hres'][0, 0, 1:]) <= PARITY).all()


# ----------------------------------------------------------------------------- 6. the lifted problem through the hard entry
@pytest.mark.parametrize('case', sq.SMALL, ids=[c.__name__ for c in sq.SMALL])
@pytest.mark.parametrize('f', sq.FACTORS)
def test_the_lifted_problem_through_the_hard_entry_agrees(case, f):
    insts = sq.instances(case, f)
    lifted = []
    for i in insts:
        L = sq.lift(i['A'], i['B'], i['H'], i['penalty'], q=i['kw']['q'], D=i['kw']['D'], d=i['kw']['d'], rows=i['kw']['rows'])
        lifted.append(dict(A=L['A'], B=L['B'], H=L['H'], N=i['N'], k0=i['k0'], x0=i['x0'], penalty=i['penalty'],
                           kw=dict(q=L['q'], Pf=i['kw']['Pf'], D=L['D'], d=L['d'], rows=L['rows'])))
    soft = run('device', sq.batch_of(insts))
    lift = run('device', sq.batch_of(lifted), penalty=None)
    mb, nd = insts[0]['B'].shape[2], insts[0]['kw']['D'].shape[1]
    e = dict(u0=relmax(lift['u0'][..., :mb], soft['u0']), X=relmax(lift['X'], soft['X']), U=relmax(lift['U'][..., :mb], soft['U']))
    es = np.abs(lift['U'][..., mb:] - soft['eps']).max() / max(1.0, np.abs(soft['lam']).max())
    print('   iters lifted %s eliminated %s | %s, slacks %.1e' % (lift['iters_total'][:, 0].tolist(), soft['iters_total'][:, 0].tolist(),
                                                              {q: '%.1e' % v for q, v in e.items()}, es))
    assert not soft['status'].any() and not lift['status'].any() and max(e.values()) <= PARITY and es <= PARITY


# ----------------------------------------------------------------------------- 7. bit-identity
def shared_penalty_batch(case, f):
    """A case as it is (ns states per problem) with one penalty per problem: that of its first instance."""
    c = case()
    nb = c['A'].shape[0]
    per = len(sq.instances(case, f)) // nb
    pen = np.stack([sq.instances(case, f)[b * per]['penalty'] for b in range(nb)])
    return dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=c['rows'].astype(np.int32), penalty=pen, N=c['N'], k0=c['k0'])


@pytest.mark.parametrize('case', [mq.case_mixed_small, mq.case_box_bench], ids=['mixed_small', 'box_bench'])
def test_without_soft_rows_the_call_is_the_existing_one_bit_for_bit(case):
    bt = shared_penalty_batch(case, 0.3)
    inf = np.full_like(bt['penalty'], np.inf)
    for entry in ENTRIES:
        plain, none, allinf = run(entry, bt, penalty=None), run(entry, dict(bt, penalty=None)), run(entry, bt, penalty=inf)
        assert_same(plain, none, OUT_KEYS); assert_same(plain, allinf, OUT_KEYS)
        assert (allinf['eps'] == 0).all() and (allinf['nviol'] == 0).all()
        plainT, allinfT = run(entry, bt, T_LOOP, penalty=None), run(entry, bt, T_LOOP, penalty=inf)
        assert_same(plainT, allinfT, LOOP_KEYS)


@pytest.mark.parametrize('case,hard_first', [(mq.case_mixed_small, True), (mq.case_box_bench, False)], ids=['mixed_small-mixed', 'box_bench'])
def test_entries_neighbours_and_absent_outputs_do_not_change_a_bit(case, hard_first):
    bt = shared_penalty_batch(case, 0.3)
    if hard_first:
        bt['penalty'][:, :, 0] = np.inf
    keys = LOOP_KEYS + ('nviol',)
    dev = run('device', bt, T_LOOP); host = run('host', bt, T_LOOP)
    assert not dev['status'].any() and dev['nviol'].sum() >= 1
    assert_same(dev, host, keys)
    assert_same(run('device', bt), run('host', bt), OUT_KEYS + ('eps', 'nviol'))
    ns = bt['X0'].shape[1]
    for s in range(min(ns, 3)):
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
    x0s = np.linspace(-6.0, 3.0, ns)
    bt, K, S, umax = scalar_batch(x0s, 3.0)
    full = run('device', bt, 3)
    assert not full['status'].any() and (full['nviol'][0, :, 0] == 1).any() and (full['nviol'][0, :, 0] == 0).any()
    for lo in range(0, ns, m.SLOTS):
        part = run('device', dict(bt, X0=np.ascontiguousarray(bt['X0'][:, lo:lo + m.SLOTS])), 3)
        for k in LOOP_KEYS + ('nviol',):
            np.testing.assert_array_equal(part[k], full[k][:, lo:lo + m.SLOTS], err_msg=k)
    want = np.array([scalar_truth(x, K, S, umax, 3.0)[0] for x in x0s])
    np.testing.assert_allclose(full['u0'][0, :, 0], want, rtol=0, atol=PARITY * max(1.0, np.abs(want).max()))


# ----------------------------------------------------------------------------- 8. failure isolation
def test_a_failing_member_stops_at_its_step_and_leaves_the_others_alone():
    """p 3, N = 1: step t sees phase t mod 3 only.  Rows: +-u_1 <= 0.2 hard, u_2 <= 0.05 soft.  Member 1: the hard pair contradicts itself at phase 1 (status 1 at
    step 1); member 2: a NaN penalty (device entry: status 3 before step 0; Python and the host entry refuse it); members 0 and 3 are sound."""
    from tunempc_amd import _lib
    base = lh.case_ragged_rows()
    nb, p, nx, mb, n = 4, 3, 3, 2, 5
    A = np.ascontiguousarray(np.broadcast_to(base['A'][0], (nb, p, nx, nx))); B = np.ascontiguousarray(np.broadcast_to(base['B'][0], (nb, p, nx, mb)))
    H = np.ascontiguousarray(np.broadcast_to(base['Hc'][0], (nb, p, n, n)))
    D = np.zeros((nb, p, 3, n)); D[:, :, 0, nx] = 1.0; D[:, :, 1, nx] = -1.0; D[:, :, 2, nx + 1] = 1.0
    d = np.full((nb, p, 3), 0.2); d[:, :, 2] = 0.05
    pen = np.full((nb, p, 3), np.inf); pen[:, :, 2] = 0.05
    d[1, 1, :2] = -1.0
    pen[2, 1, 2] = np.nan
    X0 = np.random.default_rng(8).standard_normal((nb, 2, nx))
    T = 5

    def call(idx):
        dv = [to_dev(x[idx]) for x in (A, B, H, D, d, pen, X0)]
        return to_host(_lib.mpc_qp_soft_batch_device(dv[0], dv[1], dv[2], None, None, dv[3], None, dv[4], dv[5], dv[6], 1, T, 0, 1e-10, 40, True, False))
    out = call(slice(None))
    st = out['info'][..., 0].astype(int); steps = out['info'][..., 1].astype(int)
    print('   status %s steps %s iters %s nviol %s' % (st.tolist(), steps.tolist(), out['iters'][:, 0].tolist(), out['nviol'][:, 0].tolist()))
    np.testing.assert_array_equal(st, np.array([[0, 0], [1, 1], [3, 3], [0, 0]]))
    np.testing.assert_array_equal(steps, np.array([[T, T], [1, 1], [0, 0], [T, T]]))
    for b, t in ((1, 1), (2, 0)):
        assert np.isfinite(out['X'][b, :, :t + 1]).all() and np.isfinite(out['U'][b, :, :t]).all() and (out['nviol'][b, :, :t] >= 0).all()
        assert np.isnan(out['X'][b, :, t + 1:]).all() and np.isnan(out['U'][b, :, t:]).all() and np.isnan(out['XT'][b]).all() and np.isnan(out['hres'][b, :, t:]).all()
        assert (out['nact'][b, :, t:] == -1).all() and (out['nviol'][b, :, t:] == -1).all() and (out['iters'][b, :, t + 1:] == -1).all()
    assert (out['iters'][1, :, 1] == 40).all() and np.isnan(out['U0'][2]).all()
    assert out['nviol'][[0, 3]].sum() >= 1
    sound = call([0, 3])
    for k in ('X', 'U', 'iters', 'nact', 'nviol', 'hres', 'XT', 'U0', 'info'):
        np.testing.assert_array_equal(sound[k], out[k][[0, 3]], err_msg=k)
    with pytest.raises(ValueError, match='penalty\\[2\\]\\[1\\]\\[2\\] = nan'):
        _lib.mpc_qp_soft_batch_host(A, B, H, None, None, D, None, d, pen, X0, 1, T, 0, 1e-10, 40, True, False)


# ----------------------------------------------------------------------------- 9. the edge of the layout
@pytest.mark.parametrize('entry', ENTRIES)
def test_the_layout_edge_runs_with_soft_rows(entry):
    from tunempc_amd import mpc_qp as m
    insts = sq.instances(mq.case_layout_edge, 0.3)
    assert m.lds_layout(40, 24, 4, soft=True)['bytes'] <= m.LDS_BYTES
    out = run(entry, sq.batch_of(insts))
    assert not out['status'].any()
    for b, i in enumerate(insts):
        lmax = max(1.0, out['lam'][b, 0].max())
        k = sq.kkt_check_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], out['X'][b, 0], out['U'][b, 0], out['lam'][b, 0], out['eps'][b, 0], i['penalty'], **i['kw'])
        print('   instance %d: iters %d nact %d nviol %d | by itself %s' % (b, out['iters_total'][b, 0], out['nact'][b, 0], out['nviol'][b, 0], {q: '%.1e' % v for q, v in k.items()}))
        assert max(k['dyn'], k['viol'], k['comp'], k['comp_e'], k['stat']) <= PARITY and k['low'] >= -PARITY * lmax, k
    # the row capacity that the hard layout accepts and the soft one does not
    nd = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    assert m.lds_layout(40, 24, nd, soft=True)['bytes'] > m.LDS_BYTES
    i = insts[0]
    D = np.zeros((1, 2, nd, 64)); D[:, :, :4] = i['kw']['D']
    d = np.ones((1, 2, nd)); d[:, :, :4] = i['kw']['d']
    f = to_dev if entry == 'device' else (lambda x: x)
    args = [f(np.ascontiguousarray(x[None])) for x in (i['A'], i['B'], i['H'], i['x0'][None])]
    kw = dict(D=f(D), d=f(d), ndcnt=f(np.full((1, 2), 4, np.int32)), Pf=f(np.ascontiguousarray(i['kw']['Pf'][None])))
    with pytest.raises(NotImplementedError, match='room for %d soft rows' % nd):
        m.mpc_qp_batch(*args, 2, penalty=f(np.ones((1, 2, nd))), **kw)


# ----------------------------------------------------------------------------- 10. the reference calling style
def test_the_reference_calling_style_with_penalty():
    from tunempc_amd import mpc_qp as m
    c = mq.case_mixed_small()
    p, nx = 3, 3
    n_i = 0
    i = sq.instances(mq.case_mixed_small, 0.3)[n_i]
    r = sq.solve_instances(mq.case_mixed_small, 0.3)[n_i]
    A, B, H = [i['A'][k] for k in range(p)], [i['B'][k] for k in range(p)], i['H']
    Q, R, Nc = [H[k, :nx, :nx] for k in range(p)], [H[k, nx:, nx:] for k in range(p)], [H[k, :nx, nx:] for k in range(p)]
    cnt = c['rows'][0]
    D = [c['D'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]; d = [c['d'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]
    pen = [i['penalty'][k, :cnt[k]] if cnt[k] else None for k in range(p)]
    kw = dict(D=D, d=d, q=[c['q'][0, k] for k in range(p)], Pf=c['Pf'][0, 0], penalty=pen)
    u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, i['x0'], c['N'], c['k0'], **kw)
    lmax = max(1.0, r['Lam'].max())
    assert info['status'] == 0 and relmax(U, r['U']) <= PARITY and relmax(X, r['X']) <= PARITY and np.abs(lam - r['Lam']).max() <= PARITY * lmax
    assert np.abs(info['eps'] - r['Eps']).max() <= PARITY * lmax and info['nviol'] == r['nviol0'] and r['b']['nviol'] >= 1
    log = m.mpc_closed_loop_sim(A, B, Q, R, Nc, i['x0'], c['N'], T_LOOP, c['k0'], **kw)
    ref = loop_reference(mq.case_mixed_small, 0.3)[n_i]
    assert set(log) >= {'x', 'u', 'l', 'h', 'usc', 'nviol'} and len(log['usc']) == len(log['h']) == T_LOOP
    assert relmax(np.array(log['x']), ref['X']) <= PARITY and relmax(np.array(log['u']), ref['U']) <= PARITY
    assert log['nact'] == ref['nact'].tolist() and log['nviol'] == ref['nviol'].tolist() and sum(log['nviol']) >= 1
    for t in range(T_LOOP):
        m_t = cnt[(c['k0'] + t) % p]
        assert log['usc'][t].shape == (m_t,) and log['h'][t].shape == (m_t,) and (log['usc'][t] >= 0).all()
        if m_t:
            assert abs(log['usc'][t].max() - max(0.0, ref['hres'][t])) <= PARITY and abs(-log['h'][t].min() - ref['hres'][t]) <= PARITY
            np.testing.assert_array_equal(log['usc'][t], np.maximum(0.0, -log['h'][t]))
    # one vector for every stage, with a hard entry; and no penalty: the log has no 'usc'
    one = dict(D=np.array([[0.0, 1.0], [0.0, -1.0]]), d=np.array([0.1, 0.1]))
    args = (np.eye(1) * 0.9, np.ones((1, 1)), np.eye(1), np.eye(1), np.zeros((1, 1)), -np.ones(1) * 3.0, 2)
    u0, X, U, lam, info = m.mpc_step(*args, penalty=np.array([0.5, np.inf]), **one)
    assert info['nviol'] == 1 and info['eps'][0, 0] > 0 and (info['eps'][:, 1] == 0).all() and abs(lam[0, 0] - 0.5) <= PARITY
    assert 'usc' not in m.mpc_closed_loop_sim(*args, 3, **one)
