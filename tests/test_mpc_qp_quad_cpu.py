"""CPU tests of the MPC step with quadratic slack penalties: the three numpy methods of tests/mpc_qp_quad_reference.py against each other (the figure that
bounds the GPU tests), the limits Z = 0 (the soft iteration) and Z -> inf (the hard solution), and what tunempc_amd.mpc_qp and the library refuse, and where
they route a call, before a device is touched.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mpc_qp_reference as mq
import mpc_qp_soft_reference as sq
import mpc_qp_quad_reference as qq

BOUND = qq.QUAD_IPM_VS_POLISH
ITERS_MAX = 25                      # measured: 6 .. 15 on the variants, 22 for the infeasible start at Z = 5e5


def _check(i, r):
    e = qq.ab_disagreement(r)
    print('   iters %d mu %.1e rp %.1e rd %.1e | margin %.2e stat %.1e active %d violated %d of %d | (a) vs (b) %s' % (
        r['a']['iters'], r['a']['mu'], r['a']['rp'], r['a']['rd'], r['b']['margin'], r['b']['stat'], r['b']['nact'], r['b']['nviol'], len(r['P']['h']),
        {k: '%.1e' % v for k, v in e.items()}))
    assert r['a']['status'] == 0 and r['a']['iters'] <= ITERS_MAX
    assert r['b']['certificate'] and r['b']['margin'] >= qq.MARGIN_MIN, r['b']['margin']
    assert max(e.values()) <= BOUND, e
    k = qq.kkt_check_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], r['X'], r['U'], r['Lam'], r['Eps'], i['penalty'], i['penalty2'], **i['kw'])
    assert max(k['dyn'], k['viol'], k['comp'], k['comp_e'], k['stat'], k['quad_v'], k['pure']) <= 1e-11 and k['low'] >= 0.0, k


@pytest.mark.parametrize('kind,case,f,zeta,hard_first', qq.VARIANTS, ids=qq.VARIANT_IDS)
def test_interior_point_with_quadratic_penalties_agrees_with_the_polished_solution(kind, case, f, zeta, hard_first):
    for i, r in zip(qq.instances(kind, case, f, zeta, hard_first), qq.solve_instances(kind, case, f, zeta, hard_first)):
        _check(i, r)
        if hard_first:                                                       # the hard rows carry no slack
            assert (r['Eps'][:, 0] == 0).all() and (r['Epsa'][:, 0] == 0).all()
        if kind == 'pure':                                                   # one pair: the slack is lam / Z, and active means violated
            assert r['b']['nviol'] == int(((r['state'] == qq.ACTIVE) & (r['cvec'] == 0)).sum())
            soft = np.isfinite(r['cvec'])
            np.testing.assert_allclose(r['b']['e'][soft], r['b']['lam'][soft] / r['zvec'][soft], rtol=0, atol=1e-15)


@pytest.mark.parametrize('c,Z', qq.INFEASIBLE, ids=['c%g-Z%g' % cz for cz in qq.INFEASIBLE])
def test_a_start_outside_a_bound_with_a_quadratic_penalty_converges(c, Z):
    i = qq.infeasible_instance(c, Z)
    assert mq.ipm(mq.dense(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], **i['kw']))['status'] == 1
    r = qq.solve_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], i['penalty2'], **i['kw'])
    _check(i, r)
    assert r['nviol0'] == 1 and abs(r['Eps'][0, 0] - 0.9) <= 1e-15
    cl = qq.closed_loop_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], 7, i['penalty'], i['penalty2'], **i['kw'])
    print('   closed loop: hres %s usc %s' % (cl['hres'], cl['usc']))
    assert cl['certificate'] and abs(cl['hres'][0] - 0.9) <= 1e-15 and abs(cl['usc'][0] - cl['hres'][0]) <= 1e-15           # hres is the slack at step 0


SMALL_VARIANTS = [(v, vid) for v, vid in zip(qq.VARIANTS, qq.VARIANT_IDS) if v[1] in qq.SMALL and not v[4]]


@pytest.mark.parametrize('kind,case,f,zeta,hard_first', [v for v, _ in SMALL_VARIANTS], ids=[vid for _, vid in SMALL_VARIANTS])
def test_eliminated_agrees_with_the_lifted_problem_through_the_hard_iteration(kind, case, f, zeta, hard_first):
    for i, r in zip(qq.instances(kind, case, f, zeta), qq.solve_instances(kind, case, f, zeta)):
        L = qq.lift_quad(i['A'], i['B'], i['H'], i['penalty'], i['penalty2'], q=i['kw']['q'], D=i['kw']['D'], d=i['kw']['d'], rows=i['kw']['rows'])
        P = mq.dense(L['A'], L['B'], L['H'], i['N'], i['k0'], i['x0'], q=L['q'], Pf=i['kw']['Pf'], D=L['D'], d=L['d'], rows=L['rows'])
        a = mq.ipm(P)
        X, Ul, _ = mq.unpack(P, a['v'])
        mb = i['B'].shape[2]
        U, E = Ul[:, :mb], Ul[:, mb:]
        rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
        e = dict(X=rel(X, r['X']), U=rel(U, r['U']), e=np.abs(E - r['Eps']).max() / max(1.0, np.abs(r['Eps']).max()))
        print('   lifted iters %d, eliminated %d | %s' % (a['iters'], r['a']['iters'], {k: '%.1e' % v for k, v in e.items()}))
        assert a['status'] == 0 and max(e.values()) <= BOUND, e
        assert rel(U, r['Ua']) <= BOUND and rel(X, r['Xa']) <= BOUND


@pytest.mark.parametrize('case,f,hard_first', [(c, f, hf) for c, f, hf in sq.VARIANTS if f != 1e3], ids=[i for i, v in zip(sq.VARIANT_IDS, sq.VARIANTS) if v[1] != 1e3])
def test_without_a_quadratic_weight_the_iteration_is_the_soft_one(case, f, hard_first):
    for i in sq.instances(case, f, hard_first):
        P = mq.dense(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], **i['kw'])
        cvec = sq.row_penalty(P, i['penalty'], i['k0'])
        a, s = qq.ipm_quad(P, cvec, np.zeros(len(cvec))), sq.ipm_soft(P, cvec)
        assert a['iters'] == s['iters'] and a['status'] == s['status'] == 0
        for k in ('v', 'lam', 's', 'e', 'nu'):
            assert np.abs(a[k] - s[k]).max() <= 1e-13 * max(1.0, np.abs(s[k]).max()), k


@pytest.mark.parametrize('case', qq.CASES, ids=[c.__name__ for c in qq.CASES])
def test_a_growing_quadratic_weight_approaches_the_hard_solution(case):
    dist = []
    for g in (1e3, 1e6, 1e9):
        worst = 0.0
        for i in qq.instances('pure', case, g):
            P = mq.dense(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], **i['kw'])
            a = qq.ipm_quad(P, sq.row_penalty(P, i['penalty'], i['k0']), sq.row_penalty(P, i['penalty2'], i['k0']))
            assert a['status'] == 0
            X, U, _ = mq.unpack(P, a['v'])
            h = i['hard']
            worst = max(worst, np.abs(X - h['X']).max() / max(1.0, np.abs(h['X']).max()), np.abs(U - h['U']).max() / max(1.0, np.abs(h['U']).max()))
        dist.append(worst)
    print('   distance to the hard solution at Z = (1e3, 1e6, 1e9) max lam: %s' % ['%.1e' % x for x in dist])
    assert dist[0] > dist[1] > dist[2]


@pytest.mark.parametrize('case', qq.CASES, ids=[c.__name__ for c in qq.CASES])
@pytest.mark.parametrize('zeta', [1.0, 100.0])
def test_a_weight_below_the_hard_multiplier_leaves_rows_with_a_slack(case, zeta):
    res = qq.solve_instances('l12', case, 0.3, zeta)
    pos = [int((r['Eps'] > 0).sum()) for r in res]
    print('   rows with e > 0 per instance:', pos)
    assert sum(pos) >= 1
    for r in res:
        vio = r['State'] == qq.VIOLATED
        assert (r['Eps'][vio] > 0).all() and (r['Eps'][~vio] == 0).all()


def test_the_constant_is_the_measured_disagreement_rounded_up():
    """QUAD_IPM_VS_POLISH: the worst (a) against (b) figure over every variant and the three infeasible starts, rounded up to one digit."""
    worst = dict(sol=0.0, lam=0.0, e=0.0); margin = np.inf
    for kind, case, f, zeta, hf in qq.VARIANTS:
        for r in qq.solve_instances(kind, case, f, zeta, hf):
            e = qq.ab_disagreement(r)
            worst = {k: max(worst[k], e[k]) for k in worst}; margin = min(margin, r['b']['margin'])
    inf = dict(sol=0.0, lam=0.0, e=0.0)
    for c, Z in qq.INFEASIBLE:
        i = qq.infeasible_instance(c, Z)
        e = qq.ab_disagreement(qq.solve_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], i['penalty2'], **i['kw']))
        inf = {k: max(inf[k], e[k]) for k in inf}
    print('   variants %s, smallest margin %.2e; infeasible starts %s' % ({k: '%.2e' % v for k, v in worst.items()}, margin, {k: '%.2e' % v for k, v in inf.items()}))
    top = max(max(worst.values()), max(inf.values()))
    assert top <= BOUND and BOUND <= 10 * top                                # rounded up to one digit, not a decade


# ----------------------------------------------------------------------------- validation and routing without a device, and without the library
@pytest.fixture
def no_library(monkeypatch):
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_the_checks_of_penalty2_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import mpc_qp as m
    z = np.zeros
    A, B, H, X0 = z((2, 3, 4, 4)), z((2, 3, 4, 2)), z((2, 3, 6, 6)), z((2, 5, 4))
    D, d, pen, Z = z((2, 3, 2, 6)), z((2, 3, 2)), np.ones((2, 3, 2)), np.ones((2, 3, 2))
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        with pytest.raises(ValueError, match='penalty2 describes the rows of D, which is None'):
            f(A, B, H, X0, 3, *extra, penalty2=Z)
        with pytest.raises(ValueError, match='penalty2 \\(2, 3, 2\\) expected, got \\(2, 3, 1\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen, penalty2=Z[..., :1])
        with pytest.raises(ValueError, match='penalty \\(2, 3, 2\\) expected, got \\(2, 3, 1\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty2=Z[..., :1])         # (penalty None: taken as zeros of the shape of penalty2)
        with pytest.raises(ValueError, match='fp64 arrays expected \\(penalty2 has dtype float32\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen, penalty2=Z.astype(np.float32))
        for bad in (-1.0, np.inf, np.nan):
            Z2 = Z.copy(); Z2[1, 2, 0] = bad
            for p_ in (pen, None):
                with pytest.raises(ValueError, match='penalty2 finite and >= 0 expected in every entry'):
                    f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=p_, penalty2=Z2)
        p2 = pen.copy(); p2[0, 1, 1] = np.inf
        with pytest.raises(ValueError, match='penalty2 = 0 expected on every hard row'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=p2, penalty2=Z)
        p2 = pen.copy(); p2[0, 1, 1] = 0.0
        Z2 = Z.copy(); Z2[0, 1, 1] = 0.0
        with pytest.raises(ValueError, match='penalty > 0 expected in every entry .*or 0 beside a penalty2 > 0'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=p2, penalty2=Z2)
        with pytest.raises(ValueError, match='penalty > 0 expected in every entry .*or 0 beside a penalty2 > 0'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty2=Z2)
        for bad in (-1.0, np.nan):
            p2 = pen.copy(); p2[1, 0, 0] = bad
            with pytest.raises(ValueError, match='penalty > 0 expected in every entry'):
                f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=p2, penalty2=Z)
        with pytest.raises(ValueError, match='penalty > 0 expected in every entry \\(inf: a hard row\\), got min 0'):      # today's error without penalty2
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen * 0)
        import torch
        with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(penalty2 differs\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen, penalty2=torch.ones((2, 3, 2), dtype=torch.float64))
    # the row capacity that the soft layout accepts and the one with Z does not
    nd = max(k for k in range(1, 400) if m.lds_layout(40, 24, k, soft=True)['bytes'] <= m.LDS_BYTES)
    assert m.lds_layout(40, 24, nd, quad=True)['bytes'] > m.LDS_BYTES
    big = (z((1, 2, 40, 40)), z((1, 2, 40, 24)), z((1, 2, 64, 64)), z((1, 1, 40)), 3)
    with pytest.raises(NotImplementedError, match='with room for %d rows with quadratic penalties per stage needs %d bytes of LDS' % (
            nd, m.lds_layout(40, 24, nd, quad=True)['bytes'])):
        m.mpc_qp_batch(*big, D=z((1, 2, nd, 64)), d=z((1, 2, nd)), penalty=np.ones((1, 2, nd)), penalty2=np.ones((1, 2, nd)))
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    with pytest.raises(ValueError, match='mpc_step: penalty2 describes the rows of D, which is None'):
        m.mpc_step(*one, penalty2=np.ones(1))
    with pytest.raises(ValueError, match='mpc_step: penalty2 must be one vector or a list of p = 1 vectors'):
        m.mpc_step(*one, D=np.ones((1, 3)), d=np.ones(1), penalty2=np.ones(2))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: penalty2 finite and >= 0 expected'):
        m.mpc_closed_loop_sim(*one, 3, D=np.ones((1, 3)), d=np.ones(1), penalty2=-np.ones(1))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: penalty > 0 expected in every entry .*or 0 beside'):
        m.mpc_closed_loop_sim(*one, 3, D=np.ones((1, 3)), d=np.ones(1), penalty=np.zeros(1), penalty2=np.zeros(1))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: penalty > 0 expected'):                                   # today's error without penalty2
        m.mpc_closed_loop_sim(*one, 3, D=np.ones((1, 3)), d=np.ones(1), penalty=np.zeros(1))


class _Routed(Exception):
    pass


def test_a_call_is_routed_to_the_quad_entry_only_with_penalty2(monkeypatch):
    """With the ten binding functions of _lib replaced by recorders: a call without penalty2 names the entry it named before, one with penalty2 the new one."""
    from tunempc_amd import _lib, mpc_qp as m
    names = ['mpc_qp_%sbatch_%s' % (lv, e) for lv in ('', 'soft_', 'eq_', 'aff_', 'quad_') for e in ('host', 'device')]
    for nm in names:
        def rec(*a, _nm=nm, **k):
            raise _Routed(_nm, a)
        monkeypatch.setattr(_lib, nm, rec)
    monkeypatch.setattr(_lib, 'load_library', lambda: (_ for _ in ()).throw(AssertionError('the library was loaded')))
    z = np.zeros
    A, B, H, X0 = z((1, 2, 3, 3)), z((1, 2, 3, 1)), z((1, 2, 4, 4)), z((1, 2, 3))
    rows = dict(D=z((1, 2, 2, 4)), d=z((1, 2, 2)))
    pen, Z = np.ones((1, 2, 2)), np.ones((1, 2, 2))
    J = z((1, 2, 1, 4))
    want = [(dict(), 'mpc_qp_batch_host'), (rows, 'mpc_qp_batch_host'), (dict(rows, penalty=pen), 'mpc_qp_soft_batch_host'),
            (dict(rows, penalty=pen, J=J), 'mpc_qp_eq_batch_host'), (dict(terminal='constraint'), 'mpc_qp_eq_batch_host'),
            (dict(rows, penalty=pen, offset=z((1, 2, 3))), 'mpc_qp_aff_batch_host'),
            (dict(rows, penalty=pen, penalty2=Z), 'mpc_qp_quad_batch_host'), (dict(rows, penalty2=Z), 'mpc_qp_quad_batch_host'),
            (dict(rows, penalty=pen, penalty2=Z * 0), 'mpc_qp_quad_batch_host'), (dict(rows, penalty=pen, penalty2=Z, J=J), 'mpc_qp_quad_batch_host'),
            (dict(rows, penalty2=Z, offset=z((1, 2, 3)), terminal='constraint'), 'mpc_qp_quad_batch_host')]
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        for kw, name in want:
            with pytest.raises(_Routed) as ei:
                f(A, B, H, X0, 3, *extra, **kw)
            got, args = ei.value.args
            assert got == name, (kw.keys(), got)
            assert ('quad' in got) == ('penalty2' in kw)
            if 'quad' in got:                                                # the arguments of the aff entry, then penalty2; penalty None -> zeros
                assert len(args) == 23 and args[14].shape == (1, 2, 2) and args[8].shape == (1, 2, 2)
                if 'penalty' not in kw:
                    assert not args[8].any()
                assert (args[13] is None) == ('offset' not in kw)
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    for kw, name in ((dict(), 'mpc_qp_batch_host'), (dict(penalty=np.ones(1)), 'mpc_qp_soft_batch_host'), (dict(penalty2=np.ones(1)), 'mpc_qp_quad_batch_host'),
                     (dict(penalty=[np.ones(1)], penalty2=[np.ones(1)]), 'mpc_qp_quad_batch_host')):
        for call in (lambda **k: m.mpc_step(*one, **k), lambda **k: m.mpc_closed_loop_sim(*one, 3, **k)):
            with pytest.raises(_Routed) as ei:
                call(D=np.ones((1, 3)), d=np.ones(1), **kw)
            assert ei.value.args[0] == name
            if 'penalty2' in kw and 'penalty' not in kw:                     # every row with Z > 0 pure quadratic
                assert ei.value.args[1][8].tolist() == [[[0.0]]]


def test_the_quad_layout_of_the_kernel_header_is_the_one_restated_in_python():
    from tunempc_amd import mpc_qp as m
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    body = src[src.index('inline MpcQpQuadLds mpc_qp_quad_layout'):src.index('struct MpcQpEqLds')]
    for term in ('l.s = mpc_qp_soft_lds(nx, mb, nd);', 'l.oZ = l.s.total;', '(long long)l.oZ + nd'):
        assert term in body, term
    assert 'double* zqv = cv + nd;' in src and 'if (QUAD) { Jl += nd; nuev += nd; reqv += nd; rrv += nd; }' in src
    assert 'MpcQpEqLds l = mpc_qp_eq_lds(nx, mb, nd, ne, true);' in src and 'l.base += nd; l.oJ += nd; l.oNu += nd; l.oReq += nd; l.oR += nd; l.total += nd;' in src
    for nx, nu, nd, N in ((24, 8, 16, 6), (3, 1, 2, 5), (40, 24, 4, 2), (5, 2, 70, 3)):
        hard, soft, quad = m.lds_layout(nx, nu, nd), m.lds_layout(nx, nu, nd, soft=True), m.lds_layout(nx, nu, nd, quad=True)
        assert soft['bytes'] == hard['bytes'] + 24 * nd and quad['bytes'] == soft['bytes'] + 8 * nd and quad['ws_doubles'](N) == soft['ws_doubles'](N)
        assert m.lds_layout(nx, nu, nd, soft=True, quad=True)['bytes'] == quad['bytes'] and m.lds_layout(nx, nu, nd, quad=False)['bytes'] == hard['bytes']
        ld = (nx + nu + 1) | 1
        eq = m.lds_layout(nx, nu, nd, soft=True, ne=3, nt=2, quad=True)
        assert eq['bytes'] == quad['bytes'] + 8 * 3 * (ld + 3) and eq['ws_doubles'](N) == soft['ws_doubles'](N) + 2 * N * 3 + 2
        assert m.lds_layout(nx, nu, nd, soft=True, ne=3, nt=2)['bytes'] == soft['bytes'] + 8 * 3 * (ld + 3)
    # the soft layout is the one it was (the figures of the parent's test)
    assert m.lds_layout(24, 8, 16, soft=True)['bytes'] == 8 * (24 * 33 + 24 * 25 + 24 * 33 + 32 * 33 + 16 * 33 + 24 * 33 + 8) + 24 * 16


def test_the_quad_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_quad_batch_host', 'tmpc_mpc_qp_quad_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 51
        decl = header[header.index('int %s(' % name):]
        assert re.sub(r'\s+', ' ', decl[:decl.index(';')]).endswith('const double* cp, const double* W, const double* penalty2)')


def test_the_quad_entries_refuse_by_themselves_what_python_refuses():
    """TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call (this machine may have no device at all)."""
    from tunempc_amd._lib import load_library
    from tunempc_amd import mpc_qp as m
    lib = load_library()
    d = (C.c_double * 64)(*([1.0] * 64))
    ok = dict(nb=1, p=2, nx=1, mb=1, nd=1, N=1, ns=1, T=1, k0=0, D=d, dd=d, tol=1e-10, it=60, A=d, U0=d, pen=d, pen2=d)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    nd_edge = max(k for k in range(1, 400) if m.lds_layout(40, 24, k, soft=True)['bytes'] <= m.LDS_BYTES)
    for f, vp in ((lib.tmpc_mpc_qp_quad_batch_host, False), (lib.tmpc_mpc_qp_quad_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(a['A']), P(d), P(d), None, None, P(a['D']), None, P(a['dd']), P(d), a['tol'], a['it'], P(a['U0']), P(d), P(d),
                     None, None, None, None, None, None, None, None, P(a['pen']), None, None, 0, None, None, None, 0, None, None, None, None,
                     None, None, None, None, None, None, None, P(a['pen2']))
        for kw in (dict(nb=0), dict(N=0), dict(T=0), dict(k0=2), dict(D=None), dict(dd=None), dict(tol=0.0), dict(it=0), dict(A=None), dict(U0=None),
                   dict(nd=0, D=None, dd=None), dict(pen=None)):
            assert call(**kw) == -1, kw
        assert b'penalty2 stands beside penalty, which is null' in lib.tmpc_last_error() and f.__name__.encode() in lib.tmpc_last_error()
        assert call(nx=40, mb=30) == -2 and b'nx + nu = 64' in lib.tmpc_last_error()
        assert call(nx=40, mb=24, nd=nd_edge) == -2                          # the soft layout fits, the one with Z does not
        msg = lib.tmpc_last_error().decode()
        assert re.search(r'needs (\d+) bytes', msg).group(1) == str(m.lds_layout(40, 24, nd_edge, quad=True)['bytes'])
    f = lib.tmpc_mpc_qp_quad_batch_host
    tail = (0, None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None)
    inf, nan = float('inf'), float('nan')
    for c, Z, txt in ((1.0, -2.0, b'penalty2[0][1][0] = -2'), (1.0, nan, b'penalty2[0][1][0] = '), (1.0, inf, b'penalty2[0][1][0] = inf'),
                      (inf, 1.0, b'0 on a hard row'), (0.0, 0.0, b'penalty[0][1][0] = 0: > 0 expected'), (-1.0, 1.0, b'penalty[0][1][0] = -1'),
                      (nan, 1.0, b'penalty[0][1][0] = ')):
        pen, pen2 = (C.c_double * 2)(1.0, c), (C.c_double * 2)(1.0, Z)
        rc = f(1, 2, 1, 1, 1, 1, 1, 1, 0, d, d, d, None, None, d, None, d, d, 1e-10, 60, d, d, d, None, None, None, None, None, None, None, None, pen, None, None,
               *tail, pen2)
        assert rc == -1 and txt in lib.tmpc_last_error() and b'tmpc_mpc_qp_quad_batch_host' in lib.tmpc_last_error(), (c, Z, lib.tmpc_last_error())
