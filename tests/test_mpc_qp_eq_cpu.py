"""CPU tests of the MPC step with equality rows and a terminal constraint: the numpy iteration (a) of tests/mpc_qp_eq_reference.py against its truth (b) (the
figure that bounds the GPU tests), (b) against the fixed-active-set law of lqr_horizon_reference, the infeasible instances, and what tunempc_amd.mpc_qp and the
library refuse before a device is touched.  No device is needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import lqr_horizon_reference as lh
import mpc_qp_eq_reference as eq

ITERS_MAX = 25                      # measured: 6 .. 11


@pytest.mark.parametrize('case', eq.VALUE_CASES, ids=[c.__name__ for c in eq.VALUE_CASES])
def test_the_iteration_agrees_with_the_polished_solution(case):
    """Measured (sol / lam / e / nu, worst instance of the case): term_box_nu1 1.5e-12 / 1.9e-11 / 0 / 1.6e-12; term_box_nu2 1.1e-10 / 3.0e-10 / 0 / 5.4e-12;
    term_p1 1.8e-13 / 3.8e-13 / 0 / 5.0e-13; term_box_bench 2.4e-11 / 2.2e-10 / 0 / 7.7e-12; tx_box_nu2 1.4e-11 / 5.6e-11 / 0 / 9.4e-14;
    rows_mixed_small 1.2e-12 / 5.7e-13 / 0 / 1.2e-12; rows_mixed_small_N2 6.5e-14 / 7.9e-15 / 0 / 6.5e-14; rows_mixed_bench 2.7e-13 / 1.4e-13 / 0 / 2.4e-13;
    edge 2.2e-14 / 2.0e-14 / 0 / 6.8e-15; soft 1.1e-13 / 1.7e-13 / 2.1e-14 / 1.2e-13.  The worst, 3.0e-10, rounded up: EQ_IPM_VS_POLISH."""
    c = case()
    active = 0
    worst = {}
    for b, rb in enumerate(eq.solve_case(c)):
        for s, r in enumerate(rb):
            d = eq.ab_disagreement(r)
            print('   %s instance %d.%d: iters %d margin %.1e nact %d nviol %d | (a) vs (b) %s' % (c['name'], b, s, r['a']['iters'], r['b']['margin'], r['b']['nact'],
                                                                                              r['b']['nviol'], {k: '%.1e' % v for k, v in d.items()}))
            assert eq.feasible(r['P']) or c['penalty'] is not None
            assert r['a']['status'] == 0 and r['a']['iters'] <= ITERS_MAX
            assert r['b']['certificate'] and r['b']['rank_ok'] and r['b']['margin'] >= eq.MARGIN_MIN, (r['b']['margin'], r['b']['stat'])
            active += r['b']['nact']
            for k, v in d.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print('   %s worst %s' % (c['name'], {k: '%.1e' % v for k, v in worst.items()}))
    assert c['D'] is None or active >= 1
    assert max(worst.values()) <= eq.EQ_IPM_VS_POLISH, worst


def test_a_dependent_equality_row_leaves_the_solution_alone():
    """The row of phase 0 stated twice: the multipliers are not defined, the solution is that of the problem with the row stated once."""
    dep, one = eq.case_dependent_row(), eq.case_rows_mixed_small()
    for rd, ro in zip(eq.solve_case(dep)[0], eq.solve_case(one)[0]):
        assert rd['a']['status'] == 0 and not rd['b']['rank_ok'] and rd['b']['sol_ok'] and ro['b']['certificate']
        e = max(np.abs(rd['Xa'] - ro['X']).max(), np.abs(rd['Ua'] - ro['U']).max(), np.abs(rd['X'] - ro['X']).max(), np.abs(rd['U'] - ro['U']).max())
        it = np.abs(rd['Xa'] - ro['Xa']).max()
        print('   dependent row: iters %d (once: %d), solution against the row stated once %.1e, iterate against iterate %.1e' % (rd['a']['iters'], ro['a']['iters'], e, it))
        assert e <= eq.EQ_IPM_VS_POLISH * max(1.0, np.abs(ro['X']).max(), np.abs(ro['U']).max())


@pytest.mark.parametrize('which', eq.LQR_CASES)
def test_without_inequality_rows_the_step_is_the_law_of_the_fixed_active_set(which):
    """(b) against u_0 = -K_0 x_0 of horizon_lqr(terminal='constraint') with the same homogeneous rows.  Measured: nu1 4.4e-16, nu2 9.4e-16, p1 2.0e-12,
    bench 1.2e-11; rounded up: EQ_POLISH_VS_LQR."""
    c = eq.case_lqr(which)
    kw = eq.kwargs(c)
    law = lh.horizon_lqr(c['A'][0], c['B'][0], c['H'][0], kw['J'], kw['erows'], c['N'], c['k0'], 'constraint', kw['Pf'])
    assert not law['infeasible'] and law['Hn0'].shape[0] == 0
    worst = 0.0
    for s, r in enumerate(eq.solve_case(c)[0]):
        u = -law['K0'] @ c['X0'][0, s]
        e = np.abs(r['U'][0] - u).max() / max(1.0, np.abs(u).max()); ea = np.abs(r['Ua'][0] - u).max() / max(1.0, np.abs(u).max())
        print('   %s instance %d: iters %d, (b) vs law %.1e, (a) vs law %.1e, |x_N| %.1e' % (which, s, r['a']['iters'], e, ea, np.abs(r['X'][-1]).max()))
        assert r['a']['status'] == 0 and r['b']['certificate']
        worst = max(worst, e)
    assert worst <= eq.EQ_POLISH_VS_LQR


def test_rows_that_cannot_be_met_end_with_status_1():
    for A, B, H, N, k0, x0, kw in eq.infeasible_instances():
        P = eq.dense_eq(A, B, H, N, k0, x0, **kw)
        a = eq.ipm_eq(P)
        print('   status %d after %d iterations, r_p %.2e' % (a['status'], a['iters'], a['rp']))
        assert not eq.feasible(P) and a['status'] == 1 and a['iters'] == 60 and a['rp'] > 1e-3


def test_the_terminal_constraint_changes_the_step():
    """The point of the rows, on the instances of term_p1 and term_box_nu2 in which a box row is active: x_N = 0 is met with the constraint and missed by more
    than 1e-2 with the terminal weight alone, and u_0 differs by more than 1e-2."""
    seen = 0
    for case in (eq.case_term_p1, eq.case_term_box_nu2):
        c = case()
        free = dict(eq.kwargs(c), Tx=None)
        for s, r0 in enumerate(eq.solve_case(c)[0]):
            if not r0['b']['nact']:
                continue
            rf = eq.solve_eq(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], c['X0'][0, s], **free)
            print('   %s instance %d: |x_N| %.1e with, %.2e without, |du_0| %.2e' % (c['name'], s, np.abs(r0['X'][-1]).max(), np.abs(rf['X'][-1]).max(),
                                                                               np.abs(r0['U'][0] - rf['U'][0]).max()))
            assert np.abs(r0['X'][-1]).max() <= eq.EQ_IPM_VS_POLISH and np.abs(rf['X'][-1]).max() > 1e-2 and np.abs(r0['U'][0] - rf['U'][0]).max() > 1e-2
            seen += 1
    assert seen >= 2


# ----------------------------------------------------------------------------- the interface, without a device
@pytest.fixture
def no_library(monkeypatch):
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_the_new_arguments_come_after_the_existing_ones():
    from tunempc_amd import mpc_qp as m
    assert list(inspect.signature(m.mpc_qp_batch).parameters)[-5:] == ['penalty', 'J', 'r', 'necnt', 'terminal']
    assert list(inspect.signature(m.mpc_closed_loop_batch).parameters)[-5:] == ['penalty', 'J', 'r', 'necnt', 'terminal']
    assert list(inspect.signature(m.mpc_step).parameters)[-4:] == ['penalty', 'J', 'r', 'terminal']
    assert list(inspect.signature(m.mpc_closed_loop_sim).parameters)[-4:] == ['penalty', 'J', 'r', 'terminal']
    assert list(inspect.signature(m.lds_layout).parameters)[:4] == ['nx', 'nu', 'nd', 'soft']


def test_the_checks_of_the_rows_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import mpc_qp as m
    z = np.zeros
    A, B, H, X0 = z((2, 3, 4, 4)), z((2, 3, 4, 2)), z((2, 3, 6, 6)), z((2, 5, 4))
    J, r, cnt = z((2, 3, 2, 6)), z((2, 3, 2)), np.ones((2, 3), np.int32)
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        with pytest.raises(ValueError, match='r describes the rows of J, which is None'):
            f(A, B, H, X0, 3, *extra, r=r)
        with pytest.raises(ValueError, match='necnt describes the rows of J, which is None'):
            f(A, B, H, X0, 3, *extra, necnt=cnt)
        with pytest.raises(ValueError, match='J \\[nb, p, ne, nx \\+ nu\\] = \\[2, 3, ne >= 1, 6\\] expected, got \\(2, 3, 2, 5\\)'):
            f(A, B, H, X0, 3, *extra, J=J[..., :5])
        with pytest.raises(ValueError, match='r \\(2, 3, 2\\) expected, got \\(2, 3, 1\\)'):
            f(A, B, H, X0, 3, *extra, J=J, r=r[..., :1])
        with pytest.raises(ValueError, match='necnt int32 \\(2, 3\\) expected'):
            f(A, B, H, X0, 3, *extra, J=J, necnt=cnt.astype(np.int64))
        with pytest.raises(ValueError, match='necnt in 0 .. ne = 2 expected, got 1 .. 3'):
            f(A, B, H, X0, 3, *extra, J=J, necnt=np.where(np.arange(3) == 1, 3, cnt).astype(np.int32))
        for bad in ('free', 0, 1.0, True):
            with pytest.raises(ValueError, match="terminal must be None, 'constraint' or an array"):
                f(A, B, H, X0, 3, *extra, terminal=bad)
        for bad in (z((2, 3, 5, 4)), z((2, 3, 0, 4)), z((2, 3, 2, 3)), z((2, 2, 4)), z((1, 3, 2, 4))):
            with pytest.raises(ValueError, match='terminal \\[nb, p, nt, nx\\] = \\[2, 3, 1 <= nt <= 4, 4\\] expected'):
                f(A, B, H, X0, 3, *extra, terminal=bad)
        with pytest.raises(ValueError, match='fp64 arrays expected \\(J has dtype float32\\)'):
            f(A, B, H, X0, 3, *extra, J=J.astype(np.float32))
        import torch
        with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(J differs\\)'):
            f(A, B, H, X0, 3, *extra, J=torch.zeros((2, 3, 2, 6), dtype=torch.float64))
        with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(terminal differs\\)'):
            f(A, B, H, X0, 3, *extra, terminal=torch.zeros((2, 3, 2, 4), dtype=torch.float64))
    # a row capacity that the plain layout accepts and the layout with equality rows refuses
    nd = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    assert m.lds_layout(40, 24, nd, ne=1)['bytes'] > m.LDS_BYTES
    big = (z((1, 2, 40, 40)), z((1, 2, 40, 24)), z((1, 2, 64, 64)), z((1, 1, 40)), 3)
    with pytest.raises(NotImplementedError, match='with room for %d rows and 1 equality rows per stage needs %d bytes of LDS' % (nd, m.lds_layout(40, 24, nd, ne=1)['bytes'])):
        m.mpc_qp_batch(*big, D=z((1, 2, nd, 64)), d=z((1, 2, nd)), J=z((1, 2, 1, 64)))
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    with pytest.raises(ValueError, match='mpc_step: r describes the rows of J, which is None'):
        m.mpc_step(*one, r=np.ones(1))
    with pytest.raises(ValueError, match='mpc_step: J\\[0\\] \\(rows, nx \\+ nu = 3\\) with r\\[0\\]'):
        m.mpc_step(*one, J=np.ones((1, 3)), r=np.ones(2))
    with pytest.raises(ValueError, match="mpc_closed_loop_sim: terminal must be 'constraint', one matrix"):
        m.mpc_closed_loop_sim(*one, 3, terminal=np.ones((1, 3)))
    with pytest.raises(ValueError, match="terminal must be None, 'constraint' or an array"):
        m.mpc_step(*one, terminal='free')


def test_the_layout_with_equality_rows_is_the_one_of_the_kernel_header():
    from tunempc_amd import mpc_qp as m
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    body = src[src.index('inline MpcQpEqLds mpc_qp_eq_lds'):src.index('__device__ __forceinline__ double mq_dot')]
    for term in ('l.base = soft ? mpc_qp_soft_lds(nx, mb, nd).total : mpc_qp_lds(nx, mb, nd).total;', 'const long long ld = ((nx + mb + 1) | 1);',
                 'oNu = (long long)l.base + (long long)ne * ld, total = oNu + 3LL * ne;',
                 'return (soft ? mpc_qp_soft_ws_doubles(nx, mb, nd, N) : mpc_qp_ws_doubles(nx, mb, nd, N)) + 2LL * N * ne + nt;'):
        assert term in body, term
    assert 'double* Jl = lds + (SOFT ? Ly.total + 3 * nd : Ly.total); double* nuev = Jl + ne * ld; double* reqv = nuev + ne; double* rrv = reqv + ne;' in src
    assert 'double* REQ = NUe + (size_t)N * ne;' in src and 'double* NUT = REQ + (size_t)N * ne;' in src
    for nx, nu, nd, N, ne, nt in ((24, 8, 16, 6, 3, 24), (3, 1, 2, 5, 0, 3), (40, 24, 4, 2, 2, 3), (5, 2, 70, 3, 9, 0)):
        ld = (nx + nu + 1) | 1
        for soft in (False, True):
            base, lay = m.lds_layout(nx, nu, nd, soft), m.lds_layout(nx, nu, nd, soft, ne=ne, nt=nt)
            assert lay['bytes'] == base['bytes'] + 8 * (ne * ld + 3 * ne) and lay['ws_doubles'](N) == base['ws_doubles'](N) + 2 * N * ne + nt
    assert m.lds_layout(24, 8, 16, ne=None)['bytes'] == m.lds_layout(24, 8, 16)['bytes']


def test_the_entries_with_equality_rows_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_eq_batch_host', 'tmpc_mpc_qp_eq_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 43
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].rstrip().endswith('int ne, const double* J,\n' + ' ' * (len(name) + 5) + 'const double* r, const int32_t* necnt, int nt, '
                                                         'const double* Tx, double* Nu, double* NuT, double* eres)')


def test_the_entries_refuse_by_themselves_what_python_refuses():
    """TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call (this machine may have no device at all)."""
    from tunempc_amd._lib import load_library
    from tunempc_amd import mpc_qp as m
    lib = load_library()
    d = (C.c_double * 64)(*([1.0] * 64))
    i = (C.c_int32 * 4)()
    ok = dict(nb=1, p=2, nx=2, mb=1, nd=1, N=1, ns=1, T=1, k0=0, ne=1, J=d, r=None, ec=None, nt=-1, Tx=None, pen=None)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    nd_edge = max(k for k in range(1, 400) if m.lds_layout(40, 24, k)['bytes'] <= m.LDS_BYTES)
    for f, vp in ((lib.tmpc_mpc_qp_eq_batch_host, False), (lib.tmpc_mpc_qp_eq_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)
        I = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: None if x is None else C.cast(x, C.POINTER(C.c_int32)))

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(d), P(d), P(d), None, None, P(d), None, P(d), P(d), 1e-10, 60, P(d), P(d), P(d),
                     None, None, None, None, None, None, None, None, P(a['pen']), None, None, a['ne'], P(a['J']), P(a['r']), I(a['ec']), a['nt'], P(a['Tx']),
                     None, None, None)
        for kw in (dict(ne=-1), dict(J=None), dict(ne=0), dict(ne=0, J=None, r=d), dict(ne=0, J=None, ec=i), dict(nt=-2), dict(nt=-1, Tx=d), dict(nt=1), dict(nt=0, Tx=d),
                   dict(nb=0)):
            assert call(**kw) == -1, kw
        assert call(nt=3, Tx=d) == -2 and b'at most nx = 2 terminal rows' in lib.tmpc_last_error()
        assert call(nx=40, mb=24, nd=nd_edge) == -2                          # the plain layout fits, the one with an equality row does not
        msg = lib.tmpc_last_error().decode()
        assert 'equality rows' in msg and re.search(r'needs (\d+) bytes', msg).group(1) == str(m.lds_layout(40, 24, nd_edge, ne=1)['bytes'])
        assert call(nx=40, mb=24, nd=nd_edge, pen=d) == -2 and b'soft rows' in lib.tmpc_last_error()
    f = lib.tmpc_mpc_qp_eq_batch_host
    cnt = (C.c_int32 * 2)(1, 2)
    assert f(1, 2, 2, 1, 1, 1, 1, 1, 0, d, d, d, None, None, d, None, d, d, 1e-10, 60, d, d, d, None, None, None, None, None, None, None, None, None, None, None,
             1, d, None, cnt, -1, None, None, None, None) == -1
    assert b'necnt[0][1] = 2 outside 0 .. ne = 1' in lib.tmpc_last_error()
