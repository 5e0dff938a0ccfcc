"""GPU tests of the periodic optimal-control QP (tunempc_amd.periodic_qp, csrc/tmpc_periodic_qp.h) against tests/periodic_qp_reference.py: every feasible
case through the batch call (numpy and torch) and through the list-style call against the polished active set, within PARITY = 10 PER_IPM_VS_POLISH; the
failing cases by status; 520 scalar problems against their closed forms; independence of the batch position; the fixed-point tie to k_mpc_qp (the orbit is
the solution of the fixed-endpoint step started on it); the hand-over to about_reference and the closed loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import periodic_qp_reference as pq  # noqa: E402
from tunempc_amd import periodic_qp as lib_pq, mpc_qp  # noqa: E402

PARITY = pq.PARITY
KEYS = ('X', 'U', 'lam', 'nu', 'pi', 'cost', 'status', 'iters', 'hres', 'eres', 'per', 'mu', 'rp', 'rd', 'pivmin')


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(o):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in o.items()}


def run(bt, device=False):
    if device:
        return to_host(lib_pq.periodic_qp_batch(**{k: (to_dev(v) if hasattr(v, 'shape') else v) for k, v in bt.items()}))
    return lib_pq.periodic_qp_batch(**bt)


def rel(x, y, sc):
    return float(np.abs(x - y).max() / sc) if np.size(y) else 0.0


def against_polish(name, o, r, b=0):
    """Member b of the output o against the polished solution r: the figures, printed, then the assertions."""
    ls = pq.mult_scale(r)
    fig = dict(X=rel(o['X'][b], r['X'], max(1.0, np.abs(r['X']).max())), U=rel(o['U'][b], r['U'], max(1.0, np.abs(r['U']).max())),
               lam=rel(o['lam'][b], r['Lam'], ls), nu=rel(o['nu'][b], r['Nu'], ls), pi=rel(o['pi'][b], r['Pi'], ls),
               cost=abs(o['cost'][b] - r['cost']) / max(1.0, abs(r['cost'])), per=float(o['per'][b]), hres=float(o['hres'][b]), eres=float(o['eres'][b]))
    print(name, 'iters', int(o['iters'][b]), {k: '%.2e' % v for k, v in fig.items()})
    assert o['status'][b] == 0 and o['steps'][b] == 1, (name, o['status'][b])
    for k in ('X', 'U', 'lam', 'nu', 'pi', 'cost', 'per', 'eres'):
        assert fig[k] <= PARITY, (name, k, fig[k])
    assert fig['hres'] <= PARITY, (name, fig['hres'])
    P = r['P']
    if len(P['h']):                                                         # the active set: lam > s with s = d - D z of the returned point
        v = np.concatenate([o['X'][b].reshape(-1), o['U'][b].reshape(-1)])
        act = o['lam'][b][P['stage'], P['row']] > P['h'] - P['G'] @ v
        assert np.array_equal(act, r['b']['active']), name


@pytest.mark.parametrize('case', pq.FEASIBLE, ids=lambda c: c.__name__)
def test_feasible_case_against_polish(case):
    c = case()
    r = pq.solve_case(c)
    bt = pq.batch_of(c)
    h = run(bt)
    d = run(bt, device=True)
    against_polish(c['name'] + ' numpy', h, r)
    against_polish(c['name'] + ' torch', d, r)
    for k in KEYS:
        np.testing.assert_array_equal(h[k], d[k], err_msg=k)
    assert abs(int(h['iters'][0]) - r['a']['iters']) <= 1
    # the list-style call: stage matrices as lists, ragged rows
    p, nx = c['A'].shape[0], c['A'].shape[1]
    kw = c['kw']
    lst = lambda M, cnt: None if M is None else [None if (cnt is not None and cnt[k] == 0) else M[k][:(M.shape[1] if cnt is None else cnt[k])] for k in range(p)]
    xref, uref, info = lib_pq.periodic_qp(list(c['A']), list(c['B']), [H[:nx, :nx] for H in c['H']], [H[nx:, nx:] for H in c['H']], [H[:nx, nx:] for H in c['H']],
                                          q=None if kw.get('q') is None else list(kw['q']), offset=None if kw.get('c') is None else list(kw['c']),
                                          D=lst(kw.get('D'), kw.get('rows')), d=lst(kw.get('d'), kw.get('rows')), J=lst(kw.get('J'), kw.get('erows')),
                                          r=lst(kw.get('r'), kw.get('erows')), periods=c['periods'])
    assert len(xref) == len(uref) == c['periods'] * p
    np.testing.assert_array_equal(np.stack(xref), h['X'][0]); np.testing.assert_array_equal(np.stack(uref), h['U'][0])
    np.testing.assert_array_equal(info['pi'], h['pi'][0]); np.testing.assert_array_equal(info['lam'], h['lam'][0])
    assert info['status'] == 0


def test_failing_cases_by_status():
    for cf, allowed in pq.FAILING:
        c = cf()
        for device in (False, True):
            o = run(pq.batch_of(c), device)
            assert int(o['status'][0]) in allowed and int(o['status'][0]) != 0 and o['steps'][0] == 0, (c['name'], o['status'])
            for k in ('X', 'U', 'lam', 'nu', 'pi', 'cost', 'hres', 'eres', 'per'):
                assert np.isnan(o[k]).all(), (c['name'], k)
    assert int(run(pq.batch_of(pq.case_not_convex()))['status'][0]) == 2
    with pytest.raises(RuntimeError, match='status'):
        lib_pq.periodic_qp(np.eye(2), np.zeros((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), offset=np.array([0.3, -0.1]))
    # a failing member between two good ones leaves them alone
    g = pq.batch_of(pq.case_no_orbit())
    good = dict(g, A=0.5 * g['A'], B=g['B'] + 1.0)
    mix = {k: (np.concatenate([good[k], g[k], good[k]]) if hasattr(g[k], 'shape') else g[k]) for k in g}
    o, alone = run(mix), run(good)
    assert list(o['status'] != 0) == [False, True, False]
    for k in KEYS:
        np.testing.assert_array_equal(o[k][0], alone[k][0], err_msg=k); np.testing.assert_array_equal(o[k][2], alone[k][0], err_msg=k)


def test_many_scalar_problems_against_their_closed_forms():
    bt, x, u, act = pq.many()
    assert bt['A'].shape[0] == 520
    for device in (False, True):
        o = run(bt, device)
        assert not o['status'].any()
        ex = np.abs(o['X'][:, 0, 0] - x) / np.maximum(1.0, np.abs(x)); eu = np.abs(o['U'][:, 0, 0] - u) / np.maximum(1.0, np.abs(u))
        print('many: worst x %.2e u %.2e, iterations %d .. %d' % (ex.max(), eu.max(), o['iters'].min(), o['iters'].max()))
        assert ex.max() <= PARITY and eu.max() <= PARITY
        assert np.array_equal(o['lam'][:, 0, 0] > bt['d'][:, 0, 0] - o['U'][:, 0, 0], act)
        assert o['per'].max() <= PARITY


def test_a_problem_does_not_depend_on_its_batch_position():
    cs = [pq.batch_of(pq.case_ragged()), pq.batch_of(pq.case_rolled())]
    alone = run(cs[0])
    other = cs[1]
    five = {k: (np.concatenate([other[k], other[k], other[k], cs[0][k], other[k]]) if hasattr(cs[0][k], 'shape') else cs[0][k]) for k in cs[0]}
    for device in (False, True):
        o = run(five, device)
        for k in KEYS:
            np.testing.assert_array_equal(o[k][3], alone[k][0], err_msg=k)


def _without_rows_on_x0_alone(bt, nx):
    """A row of stage 0 that acts on x_0 alone fixes nothing once x_0 is given (the reference moves it to the right-hand side): such a row is emptied
    (inequality: 0 <= 1; equality: 0 = 0)."""
    out = dict(bt)
    for M, rhs, fill in (('D', 'd', 1.0), ('J', 'r', 0.0)):
        if bt.get(M) is not None:
            only_x = ~bt[M][:, 0, :, nx:].any(axis=-1) & bt[M][:, 0, :, :nx].any(axis=-1)
            if only_x.any():
                out[M] = bt[M].copy(); out[M][:, 0][only_x] = 0.0
                out[rhs] = (np.zeros(bt[M].shape[:3]) if bt[rhs] is None else bt[rhs].copy()); out[rhs][:, 0][only_x] = fill
    return out


@pytest.mark.parametrize('case', [pq.case_ragged, pq.case_stage_shape], ids=lambda c: c.__name__)
def test_fixed_point_tie_to_the_mpc_step(case):
    """Fixed endpoints x_0 = x_N = x*_0 are a subset of the periodic trajectories that holds the periodic optimum, and the QP is strictly convex: the
    horizon-p step of k_mpc_qp from x*_0 with the terminal constraint x_N = x*_0 returns the orbit."""
    c = case()
    bt = pq.batch_of(c)
    p, nx = c['A'].shape[0], c['A'].shape[1]
    orb = run(bt)
    assert orb['status'][0] == 0
    x0 = orb['X'][:, :1].copy()                                             # [1, 1, nx]
    f = _without_rows_on_x0_alone(bt, nx)
    o = mpc_qp.mpc_qp_batch(bt['A'], bt['B'], bt['H'], x0, p, q=f['q'], offset=f['offset'], D=f['D'], d=f['d'], ndcnt=f['ndcnt'], J=f['J'], r=f['r'],
                            necnt=f['necnt'], terminal='constraint', terminal_rhs=np.ascontiguousarray(np.broadcast_to(x0, (1, p, nx))))
    assert o['status'][0, 0] == 0, o['status']
    X, U = o['X'][0, 0], o['U'][0, 0]
    ex = rel(X[:p], orb['X'][0], max(1.0, np.abs(orb['X']).max())); eN = rel(X[p], orb['X'][0, 0], max(1.0, np.abs(orb['X']).max()))
    eu = rel(U, orb['U'][0], max(1.0, np.abs(orb['U']).max()))
    print(c['name'], 'tie: X %.2e x_N %.2e U %.2e' % (ex, eN, eu))
    assert max(ex, eN, eu) <= PARITY


def test_hand_over_to_about_reference_and_the_closed_loop():
    """The orbit as xref, uref of about_reference: a deviation problem (cost 1/2 dw' H dw, the rows of the case with 0.1 of room around the orbit) in absolute
    coordinates; the closed loop started on the orbit stays on it for p steps."""
    c = pq.case_ragged()
    bt = pq.batch_of(c)
    p, nx = c['A'].shape[0], c['A'].shape[1]
    orb = run(bt)
    xref, uref = orb['X'][:, :p], orb['U'][:, :p]
    w = np.concatenate([xref, uref], axis=-1)
    room = np.maximum(bt['d'] - np.einsum('bkin,bkn->bki', bt['D'], w), 0.0) + 0.1
    kw = mpc_qp.about_reference(bt['A'], bt['B'], bt['H'], xref, uref, D=bt['D'], d=room)
    np.testing.assert_allclose(kw['offset'], bt['offset'], rtol=0, atol=PARITY)      # the orbit is a trajectory of the affine model
    o = mpc_qp.mpc_closed_loop_batch(bt['A'], bt['B'], bt['H'], np.ascontiguousarray(xref[:, :1]), 2 * p, p, ndcnt=bt['ndcnt'], **kw)
    assert o['status'][0, 0] == 0
    X, U = o['X'][0, 0], o['U'][0, 0]
    ex = rel(X[:p], xref[0], max(1.0, np.abs(xref).max())); eN = rel(X[p], xref[0, 0], max(1.0, np.abs(xref).max())); eu = rel(U, uref[0], max(1.0, np.abs(uref).max()))
    print('hand-over: X %.2e x_p %.2e U %.2e' % (ex, eN, eu))
    assert max(ex, eN, eu) <= PARITY
