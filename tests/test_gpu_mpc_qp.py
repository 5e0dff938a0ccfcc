"""GPU tests of the inequality-constrained MPC step and closed loop (csrc/tmpc_mpc_qp.h, tunempc_amd.mpc_qp) against method (b) of tests/mpc_qp_reference.py
(the polished active set with its optimality certificate), through the host and the device entry.

Bounds.  Against the reference: PARITY = 10 x IPM_VS_POLISH = 2e-8, ten times what the numpy interior-point method reaches against the same truth
(test_mpc_qp_cpu.py, where it is asserted); u0, X, U relative to max(1, max|.|), the multipliers relative to max(1, max lam).  Without rows, against
horizon_lqr_batch + closed_loop_batch on the same data: 10 x NO_ROWS_VS_LAW = 1e-13, ten times what the two numpy methods reach on it.  Bit-identity where the
kernel promises it: the two entries, an instance alone against the same instance among others, absent optional outputs, more instances than workspace slots.
Iteration counts are printed, not compared."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_horizon_reference as lh  # noqa: E402
import mpc_qp_reference as mq  # noqa: E402
from test_mpc_qp_cpu import IPM_VS_POLISH, NO_ROWS_VS_LAW, MARGIN_MIN, no_rows_loops  # noqa: E402

PARITY = 10 * IPM_VS_POLISH
ENTRIES = ['host', 'device']
T_LOOP = 7
CASES = {'box_nu1': mq.case_box_nu1, 'box_nu2': mq.case_box_nu2, 'mixed_small_N4': mq.case_mixed_small, 'mixed_small_N2': lambda: mq.case_mixed_small(2),
         'single_phase': mq.case_single_phase, 'box_bench': mq.case_box_bench, 'mixed_bench': mq.case_mixed_bench, 'layout_edge': mq.case_layout_edge}


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def run(entry, c, steps=None, states=slice(None), members=slice(None), X0=None, **kw):
    """mpc_qp_batch (steps None) or mpc_closed_loop_batch on (a slice of) a case through one entry -> dict of numpy arrays."""
    from tunempc_amd import mpc_qp as m
    f = to_dev if entry == 'device' else (lambda x: x)
    pick = lambda x: None if x is None else f(np.ascontiguousarray(x[members]))
    X0 = np.ascontiguousarray((c['X0'] if X0 is None else X0)[members][:, states])
    opt = {k: pick(c.get(k)) for k in ('D', 'd', 'ndcnt', 'q', 'Pf') if c.get(k) is not None}
    if c.get('ncnt') is not None:                                            # (the cases keep the int32 counts under the key of lqr_horizon_reference)
        opt['ndcnt'] = pick(c['ncnt'])
    args = (pick(c['A']), pick(c['B']), pick(c['H']), f(X0), c['N'])
    out = m.mpc_qp_batch(*args, c['k0'], **opt, **kw) if steps is None else m.mpc_closed_loop_batch(*args, steps, c['k0'], **opt, **kw)
    if entry == 'device':
        assert all(v is None or (isinstance(v, torch.Tensor) and v.is_cuda) for v in out.values())
    return to_host(out)


def assert_same(a, b, keys=None):
    for k in (keys or a.keys()):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@functools.lru_cache(maxsize=None)
def loop_reference(name):
    """The receding-horizon loop of method (b) for every instance of a case, computed once."""
    c = CASES[name]()
    return [[mq.closed_loop(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, T_LOOP, **mq.kwargs(c, b)) for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]


# ----------------------------------------------------------------------------- 1. the analytic case: every size is one
def scalar_case():
    a, b, umax = 0.9, 0.7, 0.25
    H = np.array([[[[2.0, 0.3], [0.3, 1.5]]]]); Pf = np.array([[[[1.2]]]])
    D = np.array([[[[0.0, 1.0], [0.0, -1.0]]]]); d = np.full((1, 1, 2), umax)
    K = (0.3 + b * 1.2 * a) / (1.5 + b * b * 1.2)
    return dict(A=np.array([[[[a]]]]), B=np.array([[[[b]]]]), H=H, Pf=Pf, D=D, d=d, N=1, k0=0, q=None, ncnt=None), K, umax


@pytest.mark.parametrize('entry', ENTRIES)
def test_the_scalar_step_is_the_clipped_linear_law(entry):
    c, K, umax = scalar_case()
    for x0 in (0.2, -0.3, 2.0, -5.0):                                        # inactive, inactive, active above, active below
        out = run(entry, c, X0=np.array([[[x0]]]))
        want = float(np.clip(-K * x0, -umax, umax))
        print('   x0 %+.1f: u0 %+.12f (want %+.12f) iters %d nact %d' % (x0, out['u0'][0, 0, 0], want, out['iters_total'][0, 0], out['nact'][0, 0]))
        assert out['status'][0, 0] == 0 and abs(out['u0'][0, 0, 0] - want) <= PARITY
        assert out['nact'][0, 0] == (1 if abs(K * x0) > umax else 0)
        assert abs(out['x1'][0, 0, 0] - (0.9 * x0 + 0.7 * out['u0'][0, 0, 0])) <= 1e-15 and out['hres'][0, 0] <= PARITY
        assert out['X'].shape == (1, 1, 2, 1) and out['U'].shape == (1, 1, 1, 1) and out['lam'].shape == (1, 1, 1, 2)


# ----------------------------------------------------------------------------- 2. the open-loop solution against method (b), and by itself
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', list(CASES))
def test_open_loop_solution_against_the_polished_active_set(entry, name):
    from tunempc_amd import mpc_qp as m
    c = CASES[name]()
    ref = mq.solve_case(c)
    out = run(entry, c)
    nb, ns = c['X0'].shape[:2]
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == 1).all()
    assert (out['iters_total'] <= m.MAX_ITER).all() and (out['iters_total'] == out['iters_max']).all() and (out['pivmin'] > 0).all()
    for b in range(nb):
        for s in range(ns):
            r = ref[b][s]
            lmax = max(1.0, np.abs(r['Lam']).max()) if r['Lam'].size else 1.0
            e = dict(u0=relmax(out['u0'][b, s], r['U'][0]), X=relmax(out['X'][b, s], r['X']), U=relmax(out['U'][b, s], r['U']),
                     lam=np.abs(out['lam'][b, s] - r['Lam']).max() / lmax if r['Lam'].size else 0.0)
            k = mq.kkt_check(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], out['X'][b, s], out['U'][b, s], out['lam'][b, s], **mq.kwargs(c, b))
            print('   %s %s state %d: iters %d (numpy %d) mu %.1e | vs (b) %s | by itself %s' % (name, entry, s, out['iters_total'][b, s], r['a']['iters'], out['mu'][b, s],
                                                                                              {q: '%.1e' % v for q, v in e.items()}, {q: '%.1e' % v for q, v in k.items()}))
            assert max(e.values()) <= PARITY, e
            assert r['b']['margin'] >= MARGIN_MIN
            np.testing.assert_array_equal(out['lam'][b, s] > MARGIN_MIN / 2, r['Lam'] > 0)
            assert out['nact'][b, s] == r['nact0']
            assert max(k['dyn'], k['viol'], k['comp'], k['stat']) <= PARITY and k['lam_min'] >= -PARITY * lmax, k
            np.testing.assert_array_equal(out['X'][b, s, 0], c['X0'][b, s]); np.testing.assert_array_equal(out['U'][b, s, 0], out['u0'][b, s])
    short = run(entry, c, return_traj=False)
    assert short['X'] is None and short['U'] is None and short['lam'] is None
    assert_same(short, out, [k for k in out if k not in ('X', 'U', 'lam')])


# ----------------------------------------------------------------------------- 3. the closed loop over T = 7 against the loop on method (b)
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', list(CASES))
def test_closed_loop_against_the_loop_on_the_polished_active_set(entry, name):
    c = CASES[name]()
    ref = loop_reference(name)
    out = run(entry, c, T_LOOP)
    nb, ns = c['X0'].shape[:2]
    assert out['X'].shape == (nb, ns, T_LOOP + 1, c['A'].shape[2]) and out['U'].shape == (nb, ns, T_LOOP, c['B'].shape[3]) and out['iters'].shape == (nb, ns, T_LOOP)
    assert not out['status'].any() and (out['steps'] == T_LOOP).all() and (out['iters'] <= 60).all() and (out['iters_total'] == out['iters'].sum(axis=2)).all()
    for b in range(nb):
        for s in range(ns):
            r = ref[b][s]
            assert r['certificate'] and r['margin'] >= MARGIN_MIN, (s, r['margin'])
            fin = np.isfinite(r['hres'])
            e = dict(X=relmax(out['X'][b, s], r['X']), U=relmax(out['U'][b, s], r['U']), hres=relmax(out['hres'][b, s][fin], r['hres'][fin]))
            print('   %s %s state %d: iters %s nact %s | %s' % (name, entry, s, out['iters'][b, s].tolist(), out['nact'][b, s].tolist(), {q: '%.1e' % v for q, v in e.items()}))
            assert max(e.values()) <= PARITY, e
            np.testing.assert_array_equal(out['nact'][b, s], r['nact'])
            np.testing.assert_array_equal(np.isneginf(out['hres'][b, s]), ~fin)
            np.testing.assert_array_equal(out['X'][b, s, T_LOOP], out['XT'][b, s])
    one = run(entry, c)
    np.testing.assert_array_equal(one['u0'], out['u0']); np.testing.assert_array_equal(out['U'][:, :, 0], out['u0'])
    short = run(entry, c, T_LOOP, return_traj=False)
    assert short['X'] is None and short['U'] is None
    assert_same(short, out, [k for k in out if k not in ('X', 'U')])


# ----------------------------------------------------------------------------- 4. without rows: the LQ kernels on the same data; rows far away
def test_without_rows_the_loop_is_the_rollout_of_the_horizon_gains():
    from tunempc_amd import lqr, closed_loop as cl, mpc_qp as m
    for name, A, B, H, Pf, N, k0, X0, K in no_rows_loops():
        dv = [to_dev(x[None]) for x in (A, B, H, X0, Pf)]
        g = lqr.horizon_lqr_batch(dv[0], dv[1], dv[2], N, terminal='cost', Pf=dv[4])
        law = to_host(cl.closed_loop_batch(dv[0], dv[1], g['K0'], dv[3], T_LOOP, k0))
        out = to_host(m.mpc_closed_loop_batch(dv[0], dv[1], dv[2], dv[3], N, T_LOOP, k0, Pf=dv[4]))
        e = max(relmax(out['X'], law['X']), relmax(out['U'], law['U']))
        print('   %s: GPU QP loop against GPU law rollout %.1e, iters %s' % (name, e, out['iters'][0, 0].tolist()))
        assert not out['status'].any() and (out['nact'] == 0).all() and np.isneginf(out['hres']).all()
        assert e <= 10 * NO_ROWS_VS_LAW
        # rows that are far away (d = 1e6) change nothing beyond the parity bound
        n = A.shape[1] + B.shape[2]
        D = np.random.default_rng(4).standard_normal((1, A.shape[0], 3, n))
        far = to_host(m.mpc_closed_loop_batch(dv[0], dv[1], dv[2], dv[3], N, T_LOOP, k0, Pf=dv[4], D=to_dev(D), d=to_dev(np.full(D.shape[:3], 1e6))))
        e = max(relmax(far['X'], law['X']), relmax(far['U'], law['U']))
        print('   %s: with rows at 1e6 %.1e, iters %s' % (name, e, far['iters'][0, 0].tolist()))
        assert not far['status'].any() and (far['nact'] == 0).all() and e <= PARITY


# ----------------------------------------------------------------------------- 5. bit-identity
@pytest.mark.parametrize('name', ['mixed_small_N4', 'box_bench'])
def test_entries_neighbours_and_absent_outputs_do_not_change_a_bit(name):
    c = CASES[name]()
    dev = run('device', c, T_LOOP); host = run('host', c, T_LOOP)
    assert_same(dev, host)
    assert_same(run('device', c), run('host', c))
    ns = c['X0'].shape[1]
    for s in range(min(ns, 3)):
        alone = run('device', c, T_LOOP, states=slice(s, s + 1))
        for k in ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info'):
            np.testing.assert_array_equal(alone[k][:, 0], dev[k][:, s], err_msg='%s of state %d alone' % (k, s))
        pair = run('device', c, T_LOOP, states=slice(s, s + 2))
        np.testing.assert_array_equal(pair['X'][:, 0], dev['X'][:, s]); np.testing.assert_array_equal(pair['info'][:, 0], dev['info'][:, s])
    trio = run('device', c, states=slice(0, 3)); full = run('device', c)
    for k in ('u0', 'X', 'U', 'lam', 'info'):
        np.testing.assert_array_equal(trio[k], full[k][:, :3], err_msg=k)


def test_more_instances_than_workspace_slots():
    from tunempc_amd import mpc_qp as m
    c, K, umax = scalar_case()
    ns = m.SLOTS + 37
    X0 = np.linspace(-3.0, 3.0, ns).reshape(1, ns, 1)
    full = run('device', c, 3, X0=X0)
    assert not full['status'].any()
    for lo in range(0, ns, m.SLOTS):
        part = run('device', c, 3, X0=X0, states=slice(lo, min(ns, lo + m.SLOTS)))
        for k in ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info'):
            np.testing.assert_array_equal(part[k], full[k][:, lo:lo + m.SLOTS], err_msg=k)
    np.testing.assert_allclose(full['u0'][0, :, 0], np.clip(-K * X0[0, :, 0], -umax, umax), rtol=0, atol=PARITY)


# ----------------------------------------------------------------------------- 6. failure isolation
def test_a_failing_member_stops_at_its_step_and_leaves_the_others_alone():
    """p 3, N = 1: step t sees phase t mod 3 only.  Member 1: contradictory rows at phase 1 (status 1 at step 1); member 2: H = -I at phase 2 (status 2 at step 2);
    member 3: a NaN in D at phase 1 (status 3 at step 1); members 0 and 4 are sound."""
    base = lh.case_ragged_rows()
    nb, p, nx, mb, n = 5, 3, 3, 2, 5
    A = np.ascontiguousarray(np.broadcast_to(base['A'][0], (nb, p, nx, nx))); B = np.ascontiguousarray(np.broadcast_to(base['B'][0], (nb, p, nx, mb)))
    H = np.ascontiguousarray(np.broadcast_to(base['Hc'][0], (nb, p, n, n))).copy()
    D = np.zeros((nb, p, 2, n)); D[:, :, 0, nx] = 1.0; D[:, :, 1, nx] = -1.0
    d = np.full((nb, p, 2), 0.2)
    d[1, 1] = -1.0
    H[2, 2] = -np.eye(n)
    D[3, 1, 0, 0] = np.nan
    X0 = np.random.default_rng(8).standard_normal((nb, 2, nx))
    c = dict(A=A, B=B, H=H, D=D, d=d, X0=X0, N=1, k0=0, q=None, Pf=None, ncnt=None)
    for entry in ENTRIES:
        out = run(entry, c, 5, max_iter=40)
        print('   %s: status %s steps %s iters %s' % (entry, out['status'].tolist(), out['steps'].tolist(), out['iters'][:, 0].tolist()))
        np.testing.assert_array_equal(out['status'], np.array([[0, 0], [1, 1], [2, 2], [3, 3], [0, 0]]))
        np.testing.assert_array_equal(out['steps'], np.array([[5, 5], [1, 1], [2, 2], [1, 1], [5, 5]]))
        for b, t in ((1, 1), (2, 2), (3, 1)):
            assert np.isfinite(out['X'][b, :, :t + 1]).all() and np.isfinite(out['U'][b, :, :t]).all() and (out['nact'][b, :, :t] >= 0).all()
            assert np.isnan(out['X'][b, :, t + 1:]).all() and np.isnan(out['U'][b, :, t:]).all() and np.isnan(out['XT'][b]).all() and np.isnan(out['hres'][b, :, t:]).all()
            assert (out['nact'][b, :, t:] == -1).all() and (out['iters'][b, :, t + 1:] == -1).all() and (out['iters'][b, :, t] >= 0).all()
        assert (out['iters'][1, :, 1] == 40).all()
        sound = run(entry, c, 5, members=[0, 4], max_iter=40)
        for k in ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info'):
            np.testing.assert_array_equal(sound[k], out[k][[0, 4]], err_msg=k)
    first = dict(c, k0=1)
    out = run('device', first, max_iter=40)                                  # the single step: everything of a failed member is NaN
    np.testing.assert_array_equal(out['status'][:, 0], [0, 1, 0, 3, 0])
    for b in (1, 3):
        assert np.isnan(out['u0'][b]).all() and np.isnan(out['X'][b]).all() and np.isnan(out['U'][b]).all() and np.isnan(out['lam'][b]).all() and (out['nact'][b] == -1).all()


# ----------------------------------------------------------------------------- 7. the point of the feature
def test_the_saturated_steps_differ_from_the_linear_law_and_the_free_ones_follow_it():
    from tunempc_amd import lqr, mpc_qp as m
    c = mq.case_box_bench()
    X0 = 2.0 * c['X0'][:, :1]
    ref = mq.closed_loop(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], X0[0, 0], T_LOOP, **mq.kwargs(c))
    assert ref['certificate'] and ref['margin'] >= MARGIN_MIN and ref['nact'][0] > 0 and ref['nact_all'][-1] == 0
    out = run('device', c, T_LOOP, X0=X0)
    K0 = to_host(lqr.horizon_lqr_batch(to_dev(c['A']), to_dev(c['B']), to_dev(c['H']), c['N'], terminal='cost', Pf=to_dev(c['Pf'])))['K0'][0]
    np.testing.assert_array_equal(out['nact'][0, 0], ref['nact'])
    sat = free = 0
    for t in range(T_LOOP):
        k = (c['k0'] + t) % c['A'].shape[1]
        law = -K0[k] @ out['X'][0, 0, t]
        e = np.abs(out['U'][0, 0, t] - law).max()
        print('   step %d: nact %d (horizon %d) |u - law| %.2e' % (t, ref['nact'][t], ref['nact_all'][t], e))
        if ref['nact'][t] > 0:
            assert e > 1e-2 and np.abs(out['U'][0, 0, t]).max() <= c['umax'] * (1 + PARITY); sat += 1
        elif ref['nact_all'][t] == 0:
            assert e <= PARITY * max(1.0, np.abs(law).max()); free += 1
    assert sat >= 2 and free >= 2


def test_the_reference_calling_style():
    from tunempc_amd import mpc_qp as m
    c = mq.case_mixed_small()
    p, nx = 3, 3
    A, B, H = [c['A'][0, k] for k in range(p)], [c['B'][0, k] for k in range(p)], c['H'][0]
    Q, R, Nc = [H[k, :nx, :nx] for k in range(p)], [H[k, nx:, nx:] for k in range(p)], [H[k, :nx, nx:] for k in range(p)]
    cnt = c['rows'][0]
    D = [c['D'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]; d = [c['d'][0, k, :cnt[k]] if cnt[k] else None for k in range(p)]
    kw = dict(D=D, d=d, q=[c['q'][0, k] for k in range(p)], Pf=c['Pf'][0, 0])
    x0 = c['X0'][0, 1]
    u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, x0, c['N'], c['k0'], **kw)
    r = mq.solve_case(c)[0][1]
    assert info['status'] == 0 and relmax(U, r['U']) <= PARITY and relmax(X, r['X']) <= PARITY and relmax(lam, r['Lam']) <= PARITY * max(1.0, r['Lam'].max())
    log = m.mpc_closed_loop_sim(A, B, Q, R, Nc, x0, c['N'], T_LOOP, c['k0'], **kw)
    ref = loop_reference('mixed_small_N4')[0][1]
    assert set(log) >= {'x', 'u', 'l', 'h'} and len(log['x']) == T_LOOP + 1 and len(log['u']) == len(log['l']) == len(log['h']) == T_LOOP
    assert relmax(np.array(log['x']), ref['X']) <= PARITY and relmax(np.array(log['u']), ref['U']) <= PARITY and log['nact'] == ref['nact'].tolist()
    assert all(h.shape == (cnt[(c['k0'] + t) % p],) and (h >= -PARITY).all() for t, h in enumerate(log['h']))
    with pytest.raises(RuntimeError, match='mpc_step: the solve ended with status 1'):
        m.mpc_step(np.eye(1) * 0.9, np.ones((1, 1)), np.eye(1), np.eye(1), np.zeros((1, 1)), np.ones(1), 2, D=np.array([[0.0, 1.0], [0.0, -1.0]]), d=np.array([-1.0, -1.0]))
