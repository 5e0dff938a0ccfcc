"""CPU tests of the MPC step with soft rows: the three numpy methods of tests/mpc_qp_soft_reference.py against each other (the figure that bounds the GPU
tests), the exact-penalty regime against the hard solution, the reference's rule for the weights, and what tunempc_amd.mpc_qp and the library refuse before a
device is touched.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mpc_qp_reference as mq
import mpc_qp_soft_reference as sq

BOUND = sq.SOFT_IPM_VS_POLISH
ITERS_MAX = 25                      # measured: 6 .. 14


@pytest.mark.parametrize('case,f,hard_first', sq.VARIANTS, ids=sq.VARIANT_IDS)
def test_eliminated_interior_point_agrees_with_the_polished_three_state_solution(case, f, hard_first):
    insts = sq.instances(case, f, hard_first)
    for i, r in zip(insts, sq.solve_instances(case, f, hard_first)):
        e = sq.ab_disagreement(r)
        print('   iters %d mu %.1e rp %.1e rd %.1e | margin %.2e stat %.1e active %d violated %d of %d | (a) vs (b) %s' % (
            r['a']['iters'], r['a']['mu'], r['a']['rp'], r['a']['rd'], r['b']['margin'], r['b']['stat'], r['b']['nact'], r['b']['nviol'], len(r['P']['h']),
            {k: '%.1e' % v for k, v in e.items()}))
        assert r['a']['status'] == 0 and r['a']['iters'] <= ITERS_MAX
        assert r['b']['certificate'] and r['b']['margin'] >= sq.MARGIN_MIN, r['b']['margin']
        assert max(e.values()) <= BOUND, e
        k = sq.kkt_check_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], r['X'], r['U'], r['Lam'], r['Eps'], i['penalty'], **i['kw'])
        assert max(k['dyn'], k['viol'], k['comp'], k['comp_e'], k['stat']) <= 1e-11 and k['low'] >= 0.0, k
        if hard_first:                                                       # the hard rows carry no slack
            assert (r['Eps'][:, 0] == 0).all() and (r['Epsa'][:, 0] == 0).all()


@pytest.mark.parametrize('case', sq.SMALL, ids=[c.__name__ for c in sq.SMALL])
@pytest.mark.parametrize('f', sq.FACTORS)
def test_eliminated_agrees_with_the_lifted_problem_through_the_hard_iteration(case, f):
    for i, r in zip(sq.instances(case, f), sq.solve_instances(case, f)):
        L = sq.lift(i['A'], i['B'], i['H'], i['penalty'], q=i['kw']['q'], D=i['kw']['D'], d=i['kw']['d'], rows=i['kw']['rows'])
        P = mq.dense(L['A'], L['B'], L['H'], i['N'], i['k0'], i['x0'], q=L['q'], Pf=i['kw']['Pf'], D=L['D'], d=L['d'], rows=L['rows'])
        a = mq.ipm(P)
        X, Ul, _ = mq.unpack(P, a['v'])
        mb, nd = i['B'].shape[2], i['kw']['D'].shape[1]
        U, E = Ul[:, :mb], Ul[:, mb:]
        rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
        ls = max(1.0, np.abs(r['Lam']).max())
        e = dict(X=rel(X, r['X']), U=rel(U, r['U']), e=np.abs(E - r['Epsa']).max() / ls)
        print('   lifted iters %d, eliminated %d | %s' % (a['iters'], r['a']['iters'], {k: '%.1e' % v for k, v in e.items()}))
        assert a['status'] == 0 and max(e.values()) <= BOUND, e
        assert rel(U, r['Ua']) <= BOUND and rel(X, r['Xa']) <= BOUND


@pytest.mark.parametrize('case', sq.CASES, ids=[c.__name__ for c in sq.CASES])
@pytest.mark.parametrize('f', [10.0, 1e3])
def test_the_exact_penalty_reproduces_the_hard_solution_without_slack(case, f):
    for i, r in zip(sq.instances(case, f), sq.solve_instances(case, f)):
        h = i['hard']
        assert np.abs(r['X'] - h['X']).max() <= 1e-12 * max(1.0, np.abs(h['X']).max()) and np.abs(r['U'] - h['U']).max() <= 1e-12 * max(1.0, np.abs(h['U']).max())
        assert np.abs(r['Lam'] - h['Lam']).max() <= 1e-12 * max(1.0, np.abs(h['Lam']).max())
        assert (r['Eps'] == 0).all() and r['b']['nviol'] == 0


@pytest.mark.parametrize('case', sq.CASES, ids=[c.__name__ for c in sq.CASES])
def test_a_penalty_below_the_hard_multiplier_leaves_rows_violated(case):
    res = sq.solve_instances(case, 0.3)
    nv = [r['b']['nviol'] for r in res]
    print('   violated rows per instance:', nv)
    assert sum(nv) >= 1
    for r in res:
        vio = r['State'] == sq.VIOLATED
        assert (r['Eps'][vio] > 0).all() and (r['Eps'][~vio] == 0).all()


def test_a_start_outside_a_soft_bound_converges_where_the_hard_problem_does_not():
    i = sq.infeasible_instance()
    P = mq.dense(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], **i['kw'])
    assert mq.ipm(P)['status'] == 1
    r = sq.solve_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], **i['kw'])
    e = sq.ab_disagreement(r)
    print('   iters %d, margin %.2e, (a) vs (b) %s, e of stage 0 %s' % (r['a']['iters'], r['b']['margin'], e, r['Eps'][0]))
    assert r['a']['status'] == 0 and r['b']['certificate'] and r['b']['margin'] >= sq.MARGIN_MIN and max(e.values()) <= BOUND
    assert r['nviol0'] == 1 and abs(r['Eps'][0, 0] - 0.9) <= 1e-15
    cl = sq.closed_loop_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], 7, i['penalty'], **i['kw'])
    print('   closed loop: hres %s' % cl['hres'])
    assert abs(cl['hres'][0] - 0.9) <= 1e-15 and (np.abs(cl['hres'][1:]) <= 1e-12).all()           # the violation is gone after one step: x stays on the bound


def test_slack_penalty_is_the_rule_of_the_reference():
    from tunempc_amd.mpc_qp import slack_penalty
    lam = np.array([[0.0, -0.5, 0.0, -1e-3], [0.0, -2.0, 0.0, 0.0], [0.0, 0.0, 0.0, -4e-3]])
    act = [[1, 3], [1], [3]]
    inf = np.inf
    assert np.array_equal(slack_penalty(lam, act), [inf, 2e3, inf, 4.0])
    assert np.array_equal(slack_penalty(lam, act, 'active', factor=10.0), [inf, 20.0, inf, 4e-2])
    assert np.array_equal(slack_penalty(lam, act, 'all'), [inf, 2e3, inf, 4.0])                    # rows 0, 2: multiplier 0 everywhere, no weight to give
    assert np.array_equal(slack_penalty(lam, [[1], [1], []], 'active'), [inf, 2e3, inf, inf])
    assert np.array_equal(slack_penalty(lam, act, 'none'), [inf] * 4) and np.array_equal(slack_penalty(lam, None, 'all'), [inf, 2e3, inf, 4.0])
    for kw, msg in ((dict(slack_flag='some'), 'slack_flag must be'), (dict(factor=0.0), 'factor > 0'), (dict(active_set=[[4]]), 'outside 0 .. 3')):
        with pytest.raises(ValueError, match=msg):
            slack_penalty(lam, **{'active_set': act, **kw})
    with pytest.raises(ValueError, match="needs the active set"):
        slack_penalty(lam)


# ----------------------------------------------------------------------------- validation without a device, and without the library
@pytest.fixture
def no_library(monkeypatch):
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_the_checks_of_the_penalty_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import mpc_qp as m
    z = np.zeros
    A, B, H, X0 = z((2, 3, 4, 4)), z((2, 3, 4, 2)), z((2, 3, 6, 6)), z((2, 5, 4))
    D, d, pen = z((2, 3, 2, 6)), z((2, 3, 2)), np.ones((2, 3, 2))
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        with pytest.raises(ValueError, match='penalty describes the rows of D, which is None'):
            f(A, B, H, X0, 3, *extra, penalty=pen)
        with pytest.raises(ValueError, match='penalty \\(2, 3, 2\\) expected, got \\(2, 3, 1\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen[..., :1])
        with pytest.raises(ValueError, match='fp64 arrays expected \\(penalty has dtype float32\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=pen.astype(np.float32))
        for bad in (0.0, -1.0, np.nan):
            p2 = pen.copy(); p2[1, 2, 0] = bad
            with pytest.raises(ValueError, match='penalty > 0 expected in every entry'):
                f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=p2)
        import torch
        with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(penalty differs\\)'):
            f(A, B, H, X0, 3, *extra, D=D, d=d, penalty=torch.ones((2, 3, 2), dtype=torch.float64))
    # the row capacity that the hard layout accepts and the soft one does not
    nd = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    assert m.lds_layout(40, 24, nd, soft=True)['bytes'] > m.LDS_BYTES
    big = (z((1, 2, 40, 40)), z((1, 2, 40, 24)), z((1, 2, 64, 64)), z((1, 1, 40)), 3)
    with pytest.raises(NotImplementedError, match='with room for %d soft rows per stage needs %d bytes of LDS' % (nd, m.lds_layout(40, 24, nd, soft=True)['bytes'])):
        m.mpc_qp_batch(*big, D=z((1, 2, nd, 64)), d=z((1, 2, nd)), penalty=np.ones((1, 2, nd)))
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    with pytest.raises(ValueError, match='mpc_step: penalty describes the rows of D, which is None'):
        m.mpc_step(*one, penalty=np.ones(1))
    with pytest.raises(ValueError, match='mpc_step: penalty must be one vector or a list of p = 1 vectors'):
        m.mpc_step(*one, D=np.ones((1, 3)), d=np.ones(1), penalty=np.ones(2))
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: penalty > 0 expected'):
        m.mpc_closed_loop_sim(*one, 3, D=np.ones((1, 3)), d=np.ones(1), penalty=np.zeros(1))


def test_the_soft_layout_of_the_kernel_header_is_the_one_restated_in_python():
    from tunempc_amd import mpc_qp as m
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    body = src[src.index('inline MpcQpSoftLds mpc_qp_soft_lds'):src.index('__device__ __forceinline__ double mq_dot')]
    for term in ('l.h = mpc_qp_lds(nx, mb, nd);', 'l.oEs = l.h.total; l.oNu = l.oEs + nd; l.oC = l.oNu + nd;', '(long long)l.oC + nd',
                 'return mpc_qp_ws_doubles(nx, mb, nd, N) + 4LL * N * nd;'):
        assert term in body, term
    assert 'double* ev = lds + Ly.total; double* nuv = ev + nd; double* cv = nuv + nd;' in src
    assert 'double* Eg = FAC + (size_t)N * fs; double* NUg = Eg + (size_t)N * nd; double* dEg = NUg + (size_t)N * nd; double* C2g = dEg + (size_t)N * nd;' in src
    for nx, nu, nd, N in ((24, 8, 16, 6), (3, 1, 2, 5), (40, 24, 4, 2), (5, 2, 70, 3)):
        hard, soft = m.lds_layout(nx, nu, nd), m.lds_layout(nx, nu, nd, soft=True)
        assert soft['bytes'] == hard['bytes'] + 24 * nd and soft['ws_doubles'](N) == hard['ws_doubles'](N) + 4 * N * nd
        assert m.lds_layout(nx, nu, nd, soft=False)['bytes'] == hard['bytes']
    # the hard layout is the one it was (the figures of the parent's test)
    n, ld, ldp, lv = 32, 33, 25, 33
    assert m.lds_layout(24, 8, 16)['bytes'] == 8 * (24 * ld + 24 * ldp + 24 * ld + n * ld + 16 * ld + 24 * lv + 8)
    assert m.lds_layout(24, 8, 16)['ws_doubles'](6) == 2 * 7 * 32 + 6 * 6 * 16 + 6 * 24 + 6 * 8 * 33


def test_the_soft_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_soft_batch_host', 'tmpc_mpc_qp_soft_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 34
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].rstrip().endswith('double* Lam, const double* penalty, double* Eol, int32_t* nviol)')


def test_the_soft_entries_refuse_by_themselves_what_python_refuses():
    """TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call (this machine may have no device at all)."""
    from tunempc_amd._lib import load_library
    from tunempc_amd import mpc_qp as m
    lib = load_library()
    d = (C.c_double * 64)(*([1.0] * 64))
    i = (C.c_int32 * 4)()
    ok = dict(nb=1, p=2, nx=1, mb=1, nd=1, N=1, ns=1, T=1, k0=0, D=d, dd=d, cnt=None, tol=1e-10, it=60, A=d, U0=d, pen=d)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    nd_edge = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    for f, vp in ((lib.tmpc_mpc_qp_soft_batch_host, False), (lib.tmpc_mpc_qp_soft_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)
        I = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: None if x is None else C.cast(x, C.POINTER(C.c_int32)))

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(a['A']), P(d), P(d), None, None, P(a['D']), I(a['cnt']), P(a['dd']), P(d), a['tol'], a['it'], P(a['U0']), P(d), P(d),
                     None, None, None, None, None, None, None, None, P(a['pen']), None, None)
        for kw in (dict(nb=0), dict(N=0), dict(T=0), dict(k0=2), dict(D=None), dict(dd=None), dict(tol=0.0), dict(it=0), dict(A=None), dict(U0=None),
                   dict(nd=0, D=None, dd=None)):
            assert call(**kw) == -1, kw
        assert b'penalty describes the rows of D' in lib.tmpc_last_error()
        assert call(nx=40, mb=30) == -2 and b'nx + nu = 64' in lib.tmpc_last_error()
        assert call(nx=40, mb=24, nd=nd_edge) == -2                          # the hard layout fits, the soft one does not
        msg = lib.tmpc_last_error().decode()
        assert 'soft rows' in msg and re.search(r'needs (\d+) bytes', msg).group(1) == str(m.lds_layout(40, 24, nd_edge, soft=True)['bytes'])
        assert call(nx=40, mb=24, nd=nd_edge, pen=None, nb=0) == -1
    f = lib.tmpc_mpc_qp_soft_batch_host
    for bad, txt in ((0.0, b'penalty[0][1][0] = 0'), (-2.0, b'penalty[0][1][0] = -2'), (float('nan'), b'penalty[0][1][0] = ')):
        pen = (C.c_double * 2)(1.0, bad)
        assert f(1, 2, 1, 1, 1, 1, 1, 1, 0, d, d, d, None, None, d, None, d, d, 1e-10, 60, d, d, d, None, None, None, None, None, None, None, None, pen, None, None) == -1
        assert txt in lib.tmpc_last_error() and b'> 0 expected' in lib.tmpc_last_error(), lib.tmpc_last_error()
    i[0] = 2
    assert f(1, 2, 1, 1, 1, 1, 1, 1, 0, d, d, d, None, None, d, i, d, d, 1e-10, 60, d, d, d, None, None, None, None, None, None, None, None, d, None, None) == -1
    assert b'ndcnt[0][0] = 2 outside 0 .. nd = 1' in lib.tmpc_last_error()
