"""CPU tests of the soft and quadratic-slack rows of the periodic QP: the numpy reference (periodic_qp_soft_reference) against itself -- the eliminated
iteration (a) against the polished lifted problem (b) inside the measured bound, (a) against the scalar closed forms (c), every weight inf against pq.ipm
iterate for iterate, Z = 0 against the penalty-only run, the exact-penalty members against the hard solutions --, the soft layout numbers against the header
comment, the validation of tunempc_amd.periodic_qp (before the library is touched), and the two new symbols declared, exported and bound."""
import os
import re

import numpy as np
import pytest

import periodic_qp_reference as pq
import periodic_qp_soft_reference as sq
from tunempc_amd import periodic_qp as lib_pq
from tunempc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ipm_against_the_polished_lifted_problem_within_the_constant():
    worst = {}
    for case in sq.CASES:
        c = case()
        r = sq.solve_case(c)
        assert r['a']['status'] == 0, (c['name'], r['a']['status'], r['a']['iters'])
        b = r['b']
        fig = sq.ab_disagreement(r)
        print(c['name'], 'iters', r['a']['iters'], 'margin %.2e' % b['margin'], 'nviol', r['a']['nviol'], {k: '%.1e' % v for k, v in fig.items()})
        assert b['certificate'] and b['margin'] >= sq.MARGIN_MIN, (c['name'], b['margin'], b['stat'], b['eqres'])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst', {k: '%.2e' % v for k, v in worst.items()}, 'PER_SOFT_IPM_VS_POLISH', sq.PER_SOFT_IPM_VS_POLISH, 'PARITY', sq.PARITY)
    top = max(worst.values())
    assert top <= sq.PER_SOFT_IPM_VS_POLISH
    assert top > sq.PER_SOFT_IPM_VS_POLISH / 10, 'the constant is the measured figure rounded up to one digit'


def test_the_slacks_and_their_cost_are_those_of_the_lifted_problem():
    for case in sq.CASES:
        c = case()
        r = sq.solve_case(c)
        a = r['a']
        cost_a = float(0.5 * a['v'] @ r['P']['Q'] @ a['v'] + r['P']['c'] @ a['v']) + a['pcost']
        assert abs(cost_a - r['cost']) <= 1e-8 * max(1.0, abs(r['cost'])), c['name']
        assert (r['Eps'] >= -1e-12).all() and (r['Epsa'] >= 0).all(), c['name']
        viol = np.zeros(r['Eps'].shape, bool); viol[r['P']['stage'], r['P']['row']] = (a['two'] | a['pure'])
        assert a['nviol'] == int((viol & (r['Eps'] > 1e-9)).sum()), c['name']


def test_contradictory_rows_have_a_least_violating_orbit():
    c = sq.case_contradictory()
    hard = pq.ipm(pq.dense(c['A'], c['B'], c['H'], 1, **c['kw']))
    assert hard['status'] == 1 and hard['iters'] == pq.MAX_ITER
    r = sq.solve_case(c)
    assert r['a']['status'] == 0 and r['b']['certificate']
    np.testing.assert_allclose(r['X'][0, 0], -0.32, atol=1e-9)
    np.testing.assert_allclose(r['Eps'][0], [0.28, 0.02], atol=1e-9)


def test_scalar_kinds_against_their_closed_forms():
    s = pq.SCALAR
    umax = pq.case_scalar_bound()['kw']['d'][0, 0]
    seen = set()
    for case in sq.SCALAR_KINDS:
        c = case()
        r = sq.solve_case(c)
        pen = c['pen'][0, 0] if c['pen'] is not None else 0.0
        pen2 = c['pen2'][0, 0] if c['pen2'] is not None else 0.0
        x, u, e, lam = sq.scalar_soft_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'], umax, pen, pen2)
        got = (r['Xa'][0, 0], r['Ua'][0, 0], r['Epsa'][0, 0], r['Lama'][0, 0])
        print(c['name'], 'closed form', (x, u, e, lam), '(a)', got)
        np.testing.assert_allclose(got, (x, u, e, lam), atol=1e-9)
        seen.add(e > 1e-3)
    assert seen == {True, False}
    xh, uh, _ = pq.scalar_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'], umax)
    assert sq.scalar_soft_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'], umax, np.inf)[:2] == (xh, uh)
    args, x, u, e = sq.many()
    assert len(x) > 512 and (e > 1e-3).sum() > 100 and (e == 0).sum() > 100


def test_every_weight_inf_is_the_hard_iteration_iterate_for_iterate():
    for case in pq.FEASIBLE:
        c = case()
        if c['kw'].get('D') is None:
            continue
        P = pq.dense(c['A'], c['B'], c['H'], c['periods'], **c['kw'])
        for mi in (1, 3, pq.MAX_ITER):      # the iterates after 1 and 3 steps and the last one
            h = pq.ipm(P, max_iter=mi)
            a = sq.ipm_soft(P, np.full(c['kw']['d'].shape, np.inf), None, max_iter=mi)
            assert a['iters'] == h['iters'] and a['status'] == h['status'], c['name']
            for k in ('v', 'lam', 's', 'nue', 'pi', 'piper'):
                assert np.array_equal(a[k], h[k]), (c['name'], mi, k)
            assert not a['eps'].any() and a['nviol'] == 0 and a['pcost'] == 0.0


def test_penalty2_zero_is_the_penalty_only_run():
    for case in (sq.case_scalar_l1, sq.case_wide_rows, sq.case_contradictory):
        c = case()
        P = pq.dense(c['A'], c['B'], c['H'], c['periods'], **c['kw'])
        a = sq.ipm_soft(P, c['pen'], None)
        z = sq.ipm_soft(P, c['pen'], np.zeros(c['pen'].shape))
        assert a['iters'] == z['iters']
        for k in ('v', 'lam', 's', 'e', 'nu', 'pi'):
            assert np.array_equal(a[k], z[k]), (c['name'], k)


def test_the_exact_penalty_reproduces_the_hard_solution():
    for soft, hard in sq.EXACT:
        c, r, h = soft(), sq.solve_case(soft()), pq.solve_case(hard())
        assert r['a']['nviol'] == 0 and np.array_equal(r['active'], h['active']), c['name']
        fig = dict(X=np.abs(r['X'] - h['X']).max(), U=np.abs(r['U'] - h['U']).max(), lam=np.abs(r['Lam'] - h['Lam']).max(), eps=np.abs(r['Eps']).max(),
                   a=np.abs(r['Xa'] - h['X']).max())
        print(c['name'], {k: '%.1e' % v for k, v in fig.items()})
        assert max(fig['X'], fig['U'], fig['lam'], fig['eps']) <= 1e-11 * pq.mult_scale(h) and fig['a'] <= sq.PER_SOFT_IPM_VS_POLISH * max(1.0, np.abs(h['X']).max())


def test_invalid_weights_end_before_the_first_iteration():
    c = sq.case_ragged()
    P = pq.dense(c['A'], c['B'], c['H'], c['periods'], **c['kw'])
    for pen, pen2 in ((-1.0, 0.0), (np.nan, 0.0), (1.0, -1.0), (1.0, np.inf), (np.inf, 1.0), (0.0, 0.0)):
        bp, bz = c['pen'].copy(), c['pen2'].copy()
        bp[1, 1], bz[1, 1] = pen, pen2
        a = sq.ipm_soft(P, bp, bz)
        assert a['status'] == 3 and a['iters'] == 0 and a['nviol'] == -1, (pen, pen2)


def test_soft_layout_against_the_header_comment():
    text = open(os.path.join(ROOT, 'tunempc_amd', 'csrc', 'tmpc_periodic_qp.h')).read()
    m = re.search(r'The soft layout of the two shapes above, in bytes: (\d+) and (\d+)\.', text)
    w = re.search(r'nx 24 / nu 8 / nd 16 / ne 0 / N 6: (\d+)\s*//\s*doubles, nx 3 / nu 2 / nd 4 / ne 1 / N 3: (\d+)\.', text)
    assert m and w, 'the soft counts of the header comment'
    assert lib_pq.lds_bytes(24, 8, 16, 0, soft=True) == int(m.group(1)) == lib_pq.lds_bytes(24, 8, 16, 0) + 32 * 16
    assert lib_pq.lds_bytes(3, 2, 4, 1, soft=True) == int(m.group(2)) == lib_pq.lds_bytes(3, 2, 4, 1) + 32 * 4
    assert lib_pq.ws_doubles(24, 8, 16, 0, 6, soft=True) == int(w.group(1)) == lib_pq.ws_doubles(24, 8, 16, 0, 6) + 4 * 6 * 16
    assert lib_pq.ws_doubles(3, 2, 4, 1, 3, soft=True) == int(w.group(2)) == lib_pq.ws_doubles(3, 2, 4, 1, 3) + 4 * 3 * 4
    assert lib_pq.lds_bytes(24, 8, 16, 0, False) == lib_pq.lds_bytes(24, 8, 16, 0) and lib_pq.ws_doubles(3, 2, 4, 1, 3, False) == lib_pq.ws_doubles(3, 2, 4, 1, 3)


# ----------------------------------------------------------------------------- the wrappers: every refusal before the library is touched
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was touched')
    for nm in ('load_library', 'periodic_qp_batch_host', 'periodic_qp_batch_device', 'periodic_qp_soft_batch_host', 'periodic_qp_soft_batch_device'):
        monkeypatch.setattr(_lib, nm, boom)


def test_wrapper_validation(no_library):
    bt = sq.batch_of(sq.case_ragged())
    assert lib_pq.REFUSED_KEYWORDS == ('Pf', 'guess')
    for kw in ('penalty', 'penalty2'):
        for bad in (np.ones(1), bt[kw][:, :2], bt[kw][..., :3], bt[kw][0], 1.0, [1.0]):
            with pytest.raises(ValueError, match=kw):
                lib_pq.periodic_qp_batch(**dict(bt, **{kw: bad}))
        with pytest.raises(ValueError):
            lib_pq.periodic_qp_batch(**dict(bt, **{kw: bt[kw].astype(np.float32)}))
        with pytest.raises(ValueError, match=kw + ' describes the rows of D, which is None'):
            lib_pq.periodic_qp_batch(**dict(dict(bt, D=None, d=None, ndcnt=None, penalty=None, penalty2=None), **{kw: bt[kw]}))
        with pytest.raises(ValueError, match=kw + ' describes the rows of D, which is None'):
            lib_pq.periodic_qp(bt['A'][0, 0], bt['B'][0, 0], np.eye(3), np.eye(2), np.zeros((3, 2)), **{kw: 1.0})
        with pytest.raises(ValueError, match=kw):      # a ragged list that does not fit the rows of D
            lib_pq.periodic_qp([a for a in bt['A'][0]], [b for b in bt['B'][0]], [np.eye(3)] * 3, [np.eye(2)] * 3, [np.zeros((3, 2))] * 3,
                               D=[None, bt['D'][0, 1], bt['D'][0, 2, :1]], d=[None, bt['d'][0, 1], bt['d'][0, 2, :1]], **{kw: [None, np.ones(3), np.ones(1)]})
    for kw in ('Pf', 'guess'):
        with pytest.raises(ValueError, match=kw):
            lib_pq.periodic_qp_batch(**bt, **{kw: np.ones(1)})
    nx, nu = 40, 24      # the layout edge: the hard layout fits, the soft one does not
    nd = next(m for m in range(1, 4096) if lib_pq.lds_bytes(nx, nu, m, 0, True) > lib_pq.LDS_BYTES)
    assert lib_pq.lds_bytes(nx, nu, nd, 0) <= lib_pq.LDS_BYTES
    A = np.zeros((1, 1, nx, nx)); B = np.zeros((1, 1, nx, nu)); H = np.eye(nx + nu)[None, None]
    with pytest.raises(NotImplementedError, match=str(lib_pq.lds_bytes(nx, nu, nd, 0, True))):
        lib_pq.periodic_qp_batch(A, B, H, D=np.zeros((1, 1, nd, nx + nu)), d=np.ones((1, 1, nd)), penalty=np.ones((1, 1, nd)))


def test_the_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'tunempc_hip.h')).read()
    for nm in ('tmpc_periodic_qp_soft_batch_host', 'tmpc_periodic_qp_soft_batch_device'):
        assert nm in _lib.EXPORTS and 'int %s(' % nm in hdr
    assert '#define TMPC_PERIODIC_QP_SOFT_RES %d' % _lib.PERIODIC_QP_SOFT_RES_STRIDE in hdr
    assert callable(_lib.periodic_qp_soft_batch_host) and callable(_lib.periodic_qp_soft_batch_device)
    lib = _lib.load_library()      # (loading the library does not need a device)
    assert lib.tmpc_periodic_qp_soft_batch_host.argtypes is not None and len(lib.tmpc_periodic_qp_soft_batch_host.argtypes) == 31
    assert len(lib.tmpc_periodic_qp_soft_batch_device.argtypes) == 31
    assert 'penalty2' in lib_pq.periodic_qp_batch.__doc__ and 'eps' in lib_pq.periodic_qp_batch.__doc__
