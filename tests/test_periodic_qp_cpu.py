"""CPU tests of the periodic optimal-control QP: the numpy reference (periodic_qp_reference) against itself -- the interior-point iteration against the
polished active set, the scalar case against its closed form, the two-period and rolled identities, the margins and the certificate, the border elimination
of the kernel against the dense Newton direction --, the validation of tunempc_amd.periodic_qp (every refusal comes before the library is touched) and
lds_bytes against the numbers in the header's comment."""
import os
import re

import numpy as np
import pytest

import periodic_qp_reference as pq
from tunempc_amd import periodic_qp as lib_pq
from tunempc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ipm_against_polish_within_the_constant():
    worst = 0.0
    for cf in pq.FEASIBLE:
        c = cf()
        r = pq.solve_case(c)
        assert r['a']['status'] == 0, (c['name'], r['a']['status'], r['a']['iters'])
        dis = pq.ab_disagreement(r)
        print(c['name'], 'iters', r['a']['iters'], {k: '%.2e' % v for k, v in dis.items()})
        worst = max(worst, max(dis.values()))
    print('worst', worst)
    assert worst <= pq.PER_IPM_VS_POLISH
    assert pq.PARITY == 10 * pq.PER_IPM_VS_POLISH


def test_margins_and_certificates():
    for cf in pq.FEASIBLE:
        c = cf()
        b = pq.solve_case(c)['b']
        print(c['name'], 'margin %.3e' % b['margin'], 'stat %.1e' % b['stat'], 'eqres %.1e' % b['eqres'], 'active', b['nact'])
        assert b['certificate'], c['name']
        assert b['margin'] >= pq.MARGIN_MIN, (c['name'], b['margin'])
    assert pq.solve_case(pq.case_scalar_bound())['b']['nact'] == 1 and pq.solve_case(pq.case_ragged())['b']['nact'] >= 1


def test_scalar_against_its_closed_form():
    s = pq.SCALAR
    x, u, act = pq.scalar_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'])
    r = pq.solve_case(pq.case_scalar_free())
    assert not act and abs(r['X'][0, 0] - x) <= 1e-14 and abs(r['U'][0, 0] - u) <= 1e-14
    assert abs((1 - s['a']) * x - s['b'] * u - s['c']) <= 1e-15
    umax = pq.case_scalar_bound()['kw']['d'][0, 0]
    xb, ub, actb = pq.scalar_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'], umax)
    rb = pq.solve_case(pq.case_scalar_bound())
    assert actb and ub == umax and abs(rb['X'][0, 0] - xb) <= 1e-14 and abs(rb['U'][0, 0] - ub) <= 1e-14 and rb['Lam'][0, 0] > 0
    assert abs(rb['Xa'][0, 0] - xb) <= pq.PER_IPM_VS_POLISH and abs(rb['Ua'][0, 0] - ub) <= pq.PER_IPM_VS_POLISH
    _, xs, us, acts = pq.many()
    assert acts.sum() == len(acts) // 2


def test_two_periods_and_rolled_identities():
    one, two, rolled = (pq.solve_case(c()) for c in (pq.case_ragged, pq.case_two_periods, pq.case_rolled))
    for k in ('X', 'U', 'Lam', 'Nu', 'Pi'):
        sc = max(1.0, np.abs(one[k]).max())
        assert np.abs(np.tile(one[k], (2, 1)) - two[k]).max() <= 1e-12 * sc, k
        assert np.abs(np.roll(one[k], 1, axis=0) - rolled[k]).max() <= 1e-12 * sc, k
    assert abs(two['cost'] - 2 * one['cost']) <= 1e-12 * max(1.0, abs(one['cost'])) and abs(rolled['cost'] - one['cost']) <= 1e-12 * max(1.0, abs(one['cost']))


def test_the_multipliers_are_those_of_the_stated_lagrangian():
    """pi[j] = (H z_j + q + D' lam_j + J' nu_j)_x + A_j' pi[(j + 1) mod N] at every stage, the u rows vanish: the convention of the header."""
    for cf in (pq.case_ragged, pq.case_eig_one, pq.case_odd):
        c = cf()
        r = pq.solve_case(c)
        P = r['P']
        N, nx = P['N'], P['nx']
        for j in range(N):
            S = P['stages'][j]
            z = np.concatenate([r['X'][j], r['U'][j]])
            g = S['H'] @ z + S['q'] + S['D'].T @ r['Lam'][j, :len(S['d'])] + S['J'].T @ r['Nu'][j, :len(S['r'])] + S['E'].T @ r['Pi'][(j + 1) % N]
            assert np.abs(g[:nx] - r['Pi'][j]).max() <= 1e-10 and np.abs(g[nx:]).max() <= 1e-10, (c['name'], j)


def test_failing_cases_end_with_their_status():
    for cf, allowed in pq.FAILING:
        c = cf()
        a = pq.solve_case(c)['a']
        assert a['status'] in allowed and a['status'] != 0, (c['name'], a['status'])


def test_border_elimination_equals_the_dense_newton_direction():
    """newton_border (the kernel's elimination) against newton_dense at a random interior iterate.  Without equality rows the two agree to rounding; with
    them both solve a system with entries 1 / RHO = 1e12 and agree to the conditioning of that."""
    rng = np.random.default_rng(3)
    for cf in pq.FEASIBLE:
        c = cf()
        P = pq.solve_case(c)['P']
        m, me = len(P['h']), len(P['re'])
        v = 0.3 * rng.standard_normal(len(P['c'])); lam = rng.uniform(0.5, 2.0, m); s = rng.uniform(0.5, 2.0, m)
        nue = rng.standard_normal(me); pp = rng.standard_normal(P['nx']); c1 = rng.standard_normal(m)
        dd = pq.newton_dense(P, v, lam, s, nue, pp, c1)
        dv, dpi, _, _ = pq.newton_border(P, v, lam, s, nue, pp, c1)
        ev = np.abs(dd[0] - dv).max() / max(1.0, np.abs(dd[0]).max()); ep = np.abs(dd[4] - dpi).max() / max(1.0, np.abs(dd[4]).max())
        print(c['name'], 'dv %.1e dpi %.1e' % (ev, ep))
        assert max(ev, ep) <= (1e-3 if me else 1e-11), c['name']


# ----------------------------------------------------------------------------- the wrappers: every refusal before the library is touched
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the library was touched')
    for nm in ('load_library', 'periodic_qp_batch_host', 'periodic_qp_batch_device'):
        monkeypatch.setattr(_lib, nm, boom)


def _good():
    return pq.batch_of(pq.case_ragged())


def test_refused_keywords(no_library):
    bt = _good()
    for kw in ('penalty', 'penalty2', 'Pf', 'guess'):
        with pytest.raises(ValueError, match=kw):
            lib_pq.periodic_qp_batch(**bt, **{kw: np.ones(1)})
        with pytest.raises(ValueError, match=kw):
            lib_pq.periodic_qp(bt['A'][0, 0], bt['B'][0, 0], np.eye(3), np.eye(2), np.zeros((3, 2)), **{kw: 1.0})
    with pytest.raises(TypeError):
        lib_pq.periodic_qp_batch(**bt, horizon=3)


def test_wrong_shapes(no_library):
    bt = _good()
    bad = [dict(A=bt['A'][0]), dict(B=bt['B'][:, :2]), dict(H=bt['H'][..., :4]), dict(q=bt['q'][..., :4]), dict(offset=bt['offset'][:, :, :2]),
           dict(d=bt['d'][..., :3]), dict(D=None), dict(ndcnt=bt['ndcnt'].astype(np.int64)), dict(ndcnt=bt['ndcnt'] + 4), dict(J=None), dict(r=bt['r'][:, :2]),
           dict(necnt=-bt['necnt']), dict(periods=0), dict(periods=1.5), dict(tol=0.0), dict(max_iter=0), dict(A=bt['A'].astype(np.float32))]
    for ch in bad:
        with pytest.raises(ValueError):
            lib_pq.periodic_qp_batch(**dict(bt, **ch))
    with pytest.raises(ValueError, match='offset'):
        lib_pq.periodic_qp(bt['A'][0, 0], bt['B'][0, 0], np.eye(3), np.eye(2), np.zeros((3, 2)), offset=np.zeros(2))


def test_beyond_the_layout(no_library):
    nx, nu = 40, 24
    A = np.zeros((1, 1, nx, nx)); B = np.zeros((1, 1, nx, nu)); H = np.eye(nx + nu)[None, None]
    assert lib_pq.lds_bytes(nx, nu) <= lib_pq.LDS_BYTES < lib_pq.lds_bytes(nx, nu, 64, 8)
    with pytest.raises(NotImplementedError, match=str(lib_pq.lds_bytes(nx, nu, 64, 8))):
        lib_pq.periodic_qp_batch(A, B, H, D=np.zeros((1, 1, 64, nx + nu)), d=np.ones((1, 1, 64)), J=np.zeros((1, 1, 8, nx + nu)))
    with pytest.raises(NotImplementedError, match='64'):
        lib_pq.periodic_qp_batch(np.zeros((1, 1, 60, 60)), np.zeros((1, 1, 60, 5)), np.eye(65)[None, None])


def test_lds_bytes_against_the_header_comment():
    text = open(os.path.join(ROOT, 'tunempc_amd', 'csrc', 'tmpc_periodic_qp.h')).read()
    m = re.search(r'nx 24 / nu 8 / nd 16 / ne 0: (\d+);\s*//\s*nx 3 / nu 2 / nd 4 / ne 1: (\d+)\.', text)
    assert m, 'the two shapes of the header comment'
    assert lib_pq.lds_bytes(24, 8, 16, 0) == int(m.group(1)) and lib_pq.lds_bytes(3, 2, 4, 1) == int(m.group(2))
    assert lib_pq.ws_doubles(3, 2, 4, 1, 3) == 2 * 4 * 5 + 6 * 3 * 4 + 3 * 3 + 3 * 2 * 6 + 2 * 3 * 1 + 3 * 2 * 3 + 3 * 3


def test_the_module_is_exported_and_the_symbols_are_declared():
    import tunempc_amd
    assert tunempc_amd.periodic_qp is lib_pq
    assert 'tmpc_periodic_qp_batch_host' in _lib.EXPORTS and 'tmpc_periodic_qp_batch_device' in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, 'include', 'tunempc_hip.h')).read()
    assert 'int tmpc_periodic_qp_batch_host(' in hdr and 'int tmpc_periodic_qp_batch_device(' in hdr
    assert 'xref, uref' in lib_pq.periodic_qp_batch.__doc__ and 'periodic_qp' in tunempc_amd.mpc_qp.about_reference.__doc__
