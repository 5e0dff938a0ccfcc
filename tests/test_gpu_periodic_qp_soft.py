"""GPU tests of the soft and quadratic-slack rows of the periodic QP (tunempc_amd.periodic_qp with penalty= / penalty2=, k_periodic_qp<true> of
csrc/tmpc_periodic_qp.h) against tests/periodic_qp_soft_reference.py: every case against the polished lifted problem within PARITY = 10
PER_SOFT_IPM_VS_POLISH, nviol, active sets and iteration counts equal to the reference's; the scalar kinds and 520 scalar problems against their closed
forms; contradictory rows (status 1 hard, status 0 soft, the neighbours bit for bit); every weight inf against the existing entry bit for bit; penalty2 = 0
against the penalty-only call; numpy, torch and the list-style call; independence of the batch position; invalid weights; the layout edge; the fixed-point
tie through the soft MPC kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import periodic_qp_reference as pq  # noqa: E402
import periodic_qp_soft_reference as sq  # noqa: E402
from tunempc_amd import periodic_qp as lib_pq, mpc_qp  # noqa: E402

PARITY = sq.PARITY
HARD_KEYS = ('X', 'U', 'lam', 'nu', 'pi', 'cost', 'status', 'iters', 'hres', 'eres', 'per', 'mu', 'rp', 'rd', 'pivmin')
KEYS = HARD_KEYS + ('eps', 'nviol', 'pcost', 'emax')
# The fixed-point tie of the hard rows: worst distance 3.5e-11.
TIE_HARD = 3.5e-11


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


def stack(bts):
    return {k: (np.concatenate([b[k] for b in bts]) if hasattr(bts[0][k], 'shape') else bts[0][k]) for k in bts[0]}


def against_polish(name, o, r, b=0):
    """Member b of the output o against the polished lifted problem r: the figures, printed, then the assertions."""
    ls = pq.mult_scale(r)
    fig = dict(X=rel(o['X'][b], r['X'], max(1.0, np.abs(r['X']).max())), U=rel(o['U'][b], r['U'], max(1.0, np.abs(r['U']).max())),
               lam=rel(o['lam'][b], r['Lam'], ls), nu=rel(o['nu'][b], r['Nu'], ls), pi=rel(o['pi'][b], r['Pi'], ls),
               eps=rel(o['eps'][b], r['Eps'], max(1.0, np.abs(r['Eps']).max())), cost=abs(o['cost'][b] - r['cost']) / max(1.0, abs(r['cost'])),
               pcost=abs(o['pcost'][b] - r['a']['pcost']) / max(1.0, abs(r['cost'])), per=float(o['per'][b]), eres=float(o['eres'][b]))
    print(name, 'iters', int(o['iters'][b]), 'nviol', int(o['nviol'][b]), {k: '%.2e' % v for k, v in fig.items()})
    assert o['status'][b] == 0 and o['steps'][b] == 1, (name, o['status'][b])
    for k, v in fig.items():
        assert v <= PARITY, (name, k, v)
    P = r['P']
    v = np.concatenate([o['X'][b].reshape(-1), o['U'][b].reshape(-1)])
    Dz = P['G'] @ v - P['h']
    assert abs(o['hres'][b] - Dz.max()) <= 1e-12 and abs(o['emax'][b] - o['eps'][b].max()) == 0.0, name
    # the active set: lam > s, with s = d - D z + e of the returned point
    act = o['lam'][b][P['stage'], P['row']] > o['eps'][b][P['stage'], P['row']] - Dz
    assert np.array_equal(act, r['active'][P['stage'], P['row']]), name
    assert int(o['nviol'][b]) == r['a']['nviol'], (name, o['nviol'][b], r['a']['nviol'])
    assert int(o['iters'][b]) == r['a']['iters'], (name, o['iters'][b], r['a']['iters'])


def lst(M, cnt):
    """[p, rows, ...] with counts -> the ragged list of the list-style call (None: a stage without rows)."""
    return None if M is None else [None if (cnt is not None and cnt[k] == 0) else M[k][:(M.shape[1] if cnt is None else cnt[k])] for k in range(len(M))]


def list_call(c, **extra):
    nx = c['A'].shape[1]
    kw = c['kw']
    return lib_pq.periodic_qp(list(c['A']), list(c['B']), [H[:nx, :nx] for H in c['H']], [H[nx:, nx:] for H in c['H']], [H[:nx, nx:] for H in c['H']],
                              q=None if kw.get('q') is None else list(kw['q']), offset=None if kw.get('c') is None else list(kw['c']),
                              D=lst(kw.get('D'), kw.get('rows')), d=lst(kw.get('d'), kw.get('rows')), J=lst(kw.get('J'), kw.get('erows')),
                              r=lst(kw.get('r'), kw.get('erows')), periods=c['periods'], **extra)


@pytest.mark.parametrize('case', sq.CASES, ids=lambda c: c.__name__)
def test_case_against_the_polished_lifted_problem(case):
    c = case()
    r = sq.solve_case(c)
    bt = sq.batch_of(c)
    h = run(bt)
    d = run(bt, device=True)
    against_polish(c['name'] + ' numpy', h, r)
    for k in KEYS:
        np.testing.assert_array_equal(h[k], d[k], err_msg=k)
    # the list-style call: ragged weights, inf on hard rows; a stage without a weight of its own is hard
    rows = c['kw'].get('rows')
    extra = {}
    if c['pen'] is not None:
        extra['penalty'] = lst(c['pen'], rows)
    if c['pen2'] is not None:
        extra['penalty2'] = lst(c['pen2'], rows)
    xref, uref, info = list_call(c, **extra)
    np.testing.assert_array_equal(np.stack(xref), h['X'][0]); np.testing.assert_array_equal(np.stack(uref), h['U'][0])
    for k in ('pi', 'lam', 'eps', 'nviol', 'pcost', 'emax'):
        np.testing.assert_array_equal(info[k], h[k][0], err_msg=k)


def test_list_style_call_with_a_scalar_weight():
    w = sq.case_wide_rows()
    xs, us, infos = list_call(w, penalty=2.0)
    o = run(dict(sq.batch_of(w), penalty=np.full((1,) + w['pen'].shape, 2.0), penalty2=None))
    np.testing.assert_array_equal(np.stack(xs), o['X'][0]); np.testing.assert_array_equal(infos['eps'], o['eps'][0])


def test_scalar_kinds_against_their_closed_forms():
    s = pq.SCALAR
    umax = pq.case_scalar_bound()['kw']['d'][0, 0]
    for case in sq.SCALAR_KINDS:
        c = case()
        o = run(sq.batch_of(c))
        pen = c['pen'][0, 0] if c['pen'] is not None else 0.0
        pen2 = c['pen2'][0, 0] if c['pen2'] is not None else 0.0
        x, u, e, lam = sq.scalar_soft_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'], umax, pen, pen2)
        got = (o['X'][0, 0, 0], o['U'][0, 0, 0], o['eps'][0, 0, 0], o['lam'][0, 0, 0])
        print(c['name'], 'closed form', (x, u, e, lam), 'device', got)
        assert o['status'][0] == 0 and np.abs(np.subtract(got, (x, u, e, lam))).max() <= PARITY * max(1.0, abs(lam)), c['name']


def test_many_scalar_problems_of_all_kinds_against_their_closed_forms():
    bt, x, u, e = sq.many()
    assert bt['A'].shape[0] == 520                                          # more than 512 slots: the slot loop wraps
    for device in (False, True):
        o = run(bt, device)
        assert not o['status'].any()
        ex = np.abs(o['X'][:, 0, 0] - x) / np.maximum(1.0, np.abs(x)); eu = np.abs(o['U'][:, 0, 0] - u) / np.maximum(1.0, np.abs(u))
        ee = np.abs(o['eps'][:, 0, 0] - e) / np.maximum(1.0, np.abs(e))
        print('many: worst x %.2e u %.2e e %.2e, iterations %d .. %d' % (ex.max(), eu.max(), ee.max(), o['iters'].min(), o['iters'].max()))
        assert max(ex.max(), eu.max(), ee.max()) <= PARITY and o['per'].max() <= PARITY
        assert np.array_equal(o['nviol'] > 0, e > 1e-6) and np.array_equal(o['emax'], o['eps'][:, 0, 0])


def test_contradictory_rows_hard_and_soft_in_one_batch():
    c, g = sq.case_contradictory(), pq.batch_of(pq.case_eig_one())
    bad = dict(g, d=c['kw']['d'][None].copy())
    mix = stack([g, bad, g])
    alone = run(g)
    for device in (False, True):
        h = run(mix, device)
        assert list(h['status']) == [0, 1, 0] and h['iters'][1] == lib_pq.MAX_ITER
        for k in ('X', 'U', 'lam', 'pi', 'cost', 'hres', 'per'):
            assert np.isnan(h[k][1]).all(), k
        pen = np.full((3, 1, 2), np.inf); pen[1] = 50.0
        s = run(dict(mix, penalty=pen), device)
        assert list(s['status']) == [0, 0, 0] and s['nviol'][1] == 2 and s['hres'][1] > 0.25
        against_polish('contradictory in a batch', s, sq.solve_case(c), 1)
        np.testing.assert_allclose(s['X'][1, 0, 0], -0.32, atol=1e-9); np.testing.assert_allclose(s['eps'][1, 0], [0.28, 0.02], atol=1e-9)
        for k in HARD_KEYS:
            for b in (0, 2):
                np.testing.assert_array_equal(s[k][b], alone[k][0], err_msg=k); np.testing.assert_array_equal(h[k][b], alone[k][0], err_msg=k)


@pytest.mark.parametrize('case', [f for f in pq.FEASIBLE if f is not pq.case_scalar_free], ids=lambda c: c.__name__)
def test_every_weight_inf_gives_the_bits_of_the_existing_entry(case):
    """Every FEASIBLE case that has rows (scalar_free has none: a penalty without D is refused)."""
    bt = pq.batch_of(case())
    old = run(bt)
    pen = np.full(bt['d'].shape, np.inf)
    for device in (False, True):
        for extra in (dict(penalty=pen), dict(penalty=pen, penalty2=np.zeros(pen.shape))):
            o = run(dict(bt, **extra), device)
            for k in HARD_KEYS:
                np.testing.assert_array_equal(o[k], old[k], err_msg=k)
            assert not o['eps'].any() and not o['nviol'].any() and not o['pcost'].any() and not o['emax'].any()


def test_penalty2_zero_gives_the_bits_of_the_penalty_only_call():
    for case in (sq.case_wide_rows, sq.case_stage_shape, sq.case_contradictory):
        bt = sq.batch_of(case())
        a = run(dict(bt, penalty2=None)); z = run(dict(bt, penalty2=np.zeros(bt['penalty'].shape)))
        for k in KEYS:
            np.testing.assert_array_equal(a[k], z[k], err_msg=k)


def test_penalty2_alone_is_pure_quadratic_everywhere():
    bt = sq.batch_of(sq.case_wide_rows())
    z = np.full(bt['penalty'].shape, 5.0)
    a = run(dict(bt, penalty=None, penalty2=z)); b = run(dict(bt, penalty=np.zeros(z.shape), penalty2=z), device=True)
    assert a['status'][0] == 0
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_allclose(a['eps'], a['lam'] / 5.0, rtol=0, atol=1e-15)


def test_a_problem_does_not_depend_on_its_batch_position():
    cs = [sq.batch_of(sq.case_ragged()), sq.batch_of(sq.case_rolled())]
    alone = run(cs[0])
    other = cs[1]
    five = stack([other, other, other, cs[0], other])
    for device in (False, True):
        o = run(five, device)
        for k in KEYS:
            np.testing.assert_array_equal(o[k][3], alone[k][0], err_msg=k)


def test_each_invalid_weight_is_status_3_on_that_member_only():
    bt = sq.batch_of(sq.case_ragged())
    alone = run(bt)
    for pen, pen2 in ((-1.0, 0.0), (np.nan, 0.0), (1.0, -1.0), (1.0, np.inf), (1.0, np.nan), (np.inf, 1.0), (0.0, 0.0)):
        three = stack([bt, bt, bt])
        three['penalty'][1, 1, 1], three['penalty2'][1, 1, 1] = pen, pen2
        for device in (False, True):
            o = run(three, device)
            assert list(o['status']) == [0, 3, 0] and o['iters'][1] == 0 and o['nviol'][1] == -1, (pen, pen2, o['status'])
            for k in ('X', 'U', 'lam', 'nu', 'pi', 'eps', 'cost', 'hres', 'eres', 'per', 'pcost', 'emax'):
                assert np.isnan(o[k][1]).all(), (pen, pen2, k)
            for k in KEYS:
                np.testing.assert_array_equal(o[k][0], alone[k][0], err_msg=k); np.testing.assert_array_equal(o[k][2], alone[k][0], err_msg=k)


def test_the_layout_edge():
    nx, nu = 40, 24
    nd = next(m for m in range(1, 4096) if lib_pq.lds_bytes(nx, nu, m, 0, True) > lib_pq.LDS_BYTES)
    A = np.zeros((1, 1, nx, nx)); B = np.ones((1, 1, nx, nu)); H = np.eye(nx + nu)[None, None]
    D = np.zeros((1, 1, nd, nx + nu)); D[0, 0, :, nx] = 1.0
    with pytest.raises(NotImplementedError, match=str(lib_pq.lds_bytes(nx, nu, nd, 0, True))):
        lib_pq.periodic_qp_batch(A, B, H, D=D, d=np.ones((1, 1, nd)), penalty=np.ones((1, 1, nd)))
    assert lib_pq.lds_bytes(nx, nu, nd, 0) <= lib_pq.LDS_BYTES              # the hard layout of the same rows fits


@pytest.mark.parametrize('case', [sq.case_ragged, sq.case_stage_shape], ids=lambda c: c.__name__)
def test_fixed_point_tie_to_the_soft_mpc_step(case):
    """The tie of test_gpu_periodic_qp.py through the soft MPC kernels: the horizon-p step from x*_0 with the terminal constraint x_N = x*_0 and the same
    penalty / penalty2 returns the soft orbit and its slacks.  Bound: ten times the worst distance of the hard tie (3.5e-11), unless the CPU references of
    the two problems (sq.tie_cpu_distance: both iterations in numpy) lie further apart; then ten times their distance, the margin of PARITY for the device's
    order of accumulation.  stage_shape: the CPU references lie 2.04e-9 apart (X; U 1.57e-9, eps 3.2e-10 -- the weakly active row that sets
    PER_SOFT_IPM_VS_POLISH), so the bound there is 2.04e-8.  ragged_mixed has rows with Z > 0, which no CPU reference of the MPC step with a terminal
    constraint serves: it keeps the hard bound 3.5e-10."""
    c = case()
    bt = sq.batch_of(c)
    p, nx = c['A'].shape[0], c['A'].shape[1]
    assert bt['D'][:, 0, :, nx:].any(axis=-1).all() or bt['ndcnt'][0, 0] == 0      # no row of stage 0 acts on x_0 alone
    cpu = sq.tie_cpu_distance(c)
    print(c['name'], 'tie of the CPU references:', cpu)
    bound = 10.0 * max(TIE_HARD, cpu or 0.0)
    orb = run(bt)
    assert orb['status'][0] == 0
    x0 = orb['X'][:, :1].copy()
    o = mpc_qp.mpc_qp_batch(bt['A'], bt['B'], bt['H'], x0, p, q=bt['q'], offset=bt['offset'], D=bt['D'], d=bt['d'], ndcnt=bt['ndcnt'], J=bt['J'], r=bt['r'],
                            necnt=bt['necnt'], terminal='constraint', terminal_rhs=np.ascontiguousarray(np.broadcast_to(x0, (1, p, nx))),
                            penalty=bt['penalty'], penalty2=bt['penalty2'])
    assert o['status'][0, 0] == 0, o['status']
    X, U, E = o['X'][0, 0], o['U'][0, 0], o['eps'][0, 0]
    sx = max(1.0, np.abs(orb['X']).max())
    ex = rel(X[:p], orb['X'][0], sx); eN = rel(X[p], orb['X'][0, 0], sx)
    eu = rel(U, orb['U'][0], max(1.0, np.abs(orb['U']).max())); ee = rel(E, orb['eps'][0], max(1.0, np.abs(orb['eps']).max()))
    print(c['name'], 'tie: X %.2e x_N %.2e U %.2e eps %.2e (bound %.2e)' % (ex, eN, eu, ee, bound))
    assert max(ex, eN, eu, ee) <= bound
