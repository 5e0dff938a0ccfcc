"""CPU tests of the inequality-constrained MPC step: the two numpy methods of tests/mpc_qp_reference.py against each other (the figure that bounds the GPU
tests), the limits in which the QP is known in closed form, and what tunempc_amd.mpc_qp and the library refuse before a device is touched.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lqr_horizon_reference as lh
import mpc_qp_reference as mq

# (a) the interior-point method against (b) the polished active set, relative to max(1, max|.|) of (b), over the whole solution, u_0 and the multipliers.
# Measured on the cases below: at most 1.8e-10 on the solution and 1.5e-9 on the multipliers (the instance with the smallest margin, 6.3e-3).
IPM_VS_POLISH = 2e-9
MARGIN_MIN = 1e-3
ITERS_MAX = 20                      # measured: 6 .. 13
# Without rows: the receding-horizon loop of the dense KKT solve against the rollout of the horizon-N gains of lqr_horizon_reference over T = 7 steps, relative to
# max(1, max|.|) of X and U.  Measured: 3.3e-16, 2.8e-16 and 5.7e-15 on the three shapes of no_rows_loops().
NO_ROWS_VS_LAW = 1e-14
ALL_CASES = mq.CASES + [lambda: mq.case_mixed_small(2)]
IDS = [c.__name__ for c in mq.CASES] + ['case_mixed_small_N2']


@pytest.mark.parametrize('case', ALL_CASES, ids=IDS)
def test_interior_point_agrees_with_the_polished_active_set(case):
    c = case()
    for b, per_state in enumerate(mq.solve_case(c)):
        for s, r in enumerate(per_state):
            e = mq.ab_disagreement(r)
            print('   member %d state %d: iters %d mu %.1e rp %.1e rd %.1e | margin %.2e stat %.1e active %d of %d | (a) vs (b) %s' % (
                b, s, r['a']['iters'], r['a']['mu'], r['a']['rp'], r['a']['rd'], r['b']['margin'], r['b']['stat'], r['b']['nact'], len(r['P']['h']),
                {k: '%.1e' % v for k, v in e.items()}))
            assert r['a']['status'] == 0 and r['a']['iters'] <= ITERS_MAX
            assert r['b']['certificate'] and r['b']['margin'] >= MARGIN_MIN, r['b']['margin']
            assert max(e.values()) <= IPM_VS_POLISH, e
            k = mq.kkt_check(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], r['X'], r['U'], r['Lam'], **mq.kwargs(c, b))
            assert max(k['dyn'], k['viol'], k['comp'], k['stat']) <= 1e-12 and k['lam_min'] >= 0.0, k


def test_some_instance_of_every_boxed_case_saturates():
    for case in (mq.case_box_nu1, mq.case_box_nu2, mq.case_box_bench, mq.case_single_phase):
        res = mq.solve_case(case())[0]
        assert any(r['nact0'] > 0 for r in res) and sum(r['b']['nact'] for r in res) > 0, case.__name__


@pytest.mark.parametrize('rows', ['none', 'far'])
def test_without_active_rows_the_step_is_the_horizon_lqr_law(rows):
    for case, N, k0 in ((lh.case_no_rows, 5, 2), (lh.case_ragged_rows, 2, 1), (lh.case_bench_stage_shape, 3, 1)):
        c = case()
        A, B, H = c['A'][0], c['B'][0], c['Hc'][0]
        p, nx = A.shape[0], A.shape[1]
        n = nx + B.shape[2]
        Pf = np.broadcast_to(np.eye(nx), (p, nx, nx))
        K0 = lh.horizon_lqr(A, B, H, None, None, N, k0, terminal='cost', Pf=Pf)['K0']
        x0 = np.random.default_rng(3).standard_normal(nx)
        kw = dict(Pf=Pf)
        if rows == 'far':
            D = np.random.default_rng(4).standard_normal((p, 3, n))
            kw.update(D=D, d=np.full((p, 3), 1e6))
        r = mq.solve(A, B, H, N, k0, x0, **kw)
        e = np.abs(r['Ua'][0] + K0 @ x0).max() / max(1.0, np.abs(K0 @ x0).max())
        print('   %s %s: iters %d, |u_0 + K_0 x_0| %.1e' % (case.__name__, rows, r['a']['iters'], e))
        assert r['a']['status'] == 0 and r['b']['nact'] == 0 and e <= IPM_VS_POLISH


def no_rows_loops(T=7):
    """(name, A, B, H, Pf, N, k0, X0 [ns,nx], K [p,mb,nx] the horizon-N gains from every phase) of the three shapes of the no-rows comparison."""
    out = []
    for case, N, k0 in ((lh.case_no_rows, 5, 2), (lh.case_ragged_rows, 2, 1), (lh.case_bench_stage_shape, 3, 1)):
        c = case()
        A, B, H = c['A'][0], c['B'][0], c['Hc'][0]
        p, nx = A.shape[0], A.shape[1]
        Pf = np.ascontiguousarray(np.broadcast_to(np.eye(nx), (p, nx, nx)))
        K = np.stack([lh.horizon_lqr(A, B, H, None, None, N, k, terminal='cost', Pf=Pf)['K0'] for k in range(p)])
        out.append((case.__name__, A, B, H, Pf, N, k0, np.random.default_rng(21).standard_normal((2, nx)), K))
    return out


def law_rollout(A, B, K, x0, T, k0):
    X = [x0]; U = []
    for t in range(T):
        k = (k0 + t) % A.shape[0]
        U.append(-K[k] @ X[-1]); X.append(A[k] @ X[-1] + B[k] @ U[-1])
    return np.array(X), np.array(U)


def test_without_rows_the_receding_horizon_loop_is_the_rollout_of_the_gains():
    for name, A, B, H, Pf, N, k0, X0, K in no_rows_loops():
        for x0 in X0:
            r = mq.closed_loop(A, B, H, N, k0, x0, 7, Pf=Pf)
            X, U = law_rollout(A, B, K, x0, 7, k0)
            e = max(np.abs(r['X'] - X).max() / max(1.0, np.abs(X).max()), np.abs(r['U'] - U).max() / max(1.0, np.abs(U).max()))
            print('   %s: %.1e' % (name, e))
            assert e <= NO_ROWS_VS_LAW


def test_the_scalar_step_is_the_clipped_linear_law():
    a, b, umax = 0.9, 0.7, 0.25
    H = np.array([[[2.0, 0.3], [0.3, 1.5]]]); Pf = np.array([[[1.2]]])
    D = np.array([[[0.0, 1.0], [0.0, -1.0]]]); d = np.full((1, 2), umax)
    K = (H[0, 1, 0] + b * Pf[0, 0, 0] * a) / (H[0, 1, 1] + b * b * Pf[0, 0, 0])
    for x0 in (0.2, -0.3, 2.0, -5.0):
        r = mq.solve(np.array([[[a]]]), np.array([[[b]]]), H, 1, 0, np.array([x0]), Pf=Pf, D=D, d=d)
        want = np.clip(-K * x0, -umax, umax)
        assert r['b']['certificate'] and abs(r['U'][0, 0] - want) <= 1e-14 and abs(r['Ua'][0, 0] - want) <= IPM_VS_POLISH, (x0, r['U'], want)
        assert r['nact0'] == (1 if abs(K * x0) > umax else 0)


def test_the_receding_horizon_reference_saturates_first_and_then_follows_the_linear_law():
    c = mq.case_box_bench()
    A, B, H = c['A'][0], c['B'][0], c['H'][0]
    r = mq.closed_loop(A, B, H, c['N'], c['k0'], 2.0 * c['X0'][0, 0], 7, **mq.kwargs(c))
    print('   nact %s, over the horizon %s, margin %.1e' % (r['nact'].tolist(), r['nact_all'].tolist(), r['margin']))
    assert r['certificate'] and r['margin'] >= MARGIN_MIN and r['nact'][0] > 0 and r['nact_all'][-1] == 0
    assert (r['hres'] <= 1e-12).all() and np.abs(r['U']).max() <= c['umax'] * (1 + 1e-12)
    for t in range(7):
        k = (c['k0'] + t) % A.shape[0]
        K0 = lh.horizon_lqr(A, B, H, None, None, c['N'], k, terminal='cost', Pf=c['Pf'][0])['K0']
        e = np.abs(r['U'][t] + K0 @ r['X'][t]).max()
        assert e <= IPM_VS_POLISH if r['nact_all'][t] == 0 else (e > 1e-2 or r['nact'][t] == 0), (t, e)


def test_failures_of_the_reference_are_told_apart():
    A = np.array([[[0.9]]]); B = np.array([[[0.7]]]); H = np.array([[[2.0, 0.0], [0.0, 1.0]]])
    D = np.array([[[0.0, 1.0], [0.0, -1.0]]])
    P = mq.dense(A, B, H, 1, 0, np.array([1.0]), D=D, d=np.array([[-1.0, -1.0]]))
    assert mq.ipm(P)['status'] == 1                                          # u <= -1 and -u <= -1: infeasible, ends at max_iter
    assert mq.ipm(mq.dense(A, B, -H, 1, 0, np.array([1.0]), D=D, d=np.array([[1.0, 1.0]])))['status'] == 2
    Dn = D.copy(); Dn[0, 0, 1] = np.nan
    assert mq.ipm(mq.dense(A, B, H, 1, 0, np.array([1.0]), D=Dn, d=np.array([[1.0, 1.0]])))['status'] == 3


# ----------------------------------------------------------------------------- validation without a device, and without the library
def _batch(nb=2, p=3, nx=4, mb=2, ns=5):
    return np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, mb)), np.zeros((nb, p, nx + mb, nx + mb)), np.zeros((nb, ns, nx))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test."""
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_argument_checks_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import mpc_qp as m
    A, B, H, X0 = _batch()
    D, d = np.zeros((2, 3, 2, 6)), np.zeros((2, 3, 2))
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='horizon must be an int >= 1'):
            m.mpc_qp_batch(A, B, H, X0, bad)
        with pytest.raises(ValueError, match='steps must be an int >= 1'):
            m.mpc_closed_loop_batch(A, B, H, X0, 3, bad)
    for bad in (-1, 3, 0.0, None):
        with pytest.raises(ValueError, match='phase0 must be an int in 0 .. p - 1 = 2'):
            m.mpc_qp_batch(A, B, H, X0, 3, phase0=bad)
    with pytest.raises(ValueError, match='H \\(2, 3, 6, 6\\) expected'):
        m.mpc_qp_batch(A, B, H[:, :, :5], X0, 3)
    with pytest.raises(ValueError, match='X0 \\[nb, ns, nx\\] = \\[2, ns, 4\\] expected'):
        m.mpc_qp_batch(A, B, H, X0[:, :, :3], 3)
    with pytest.raises(ValueError, match='ns >= 1 initial states expected'):
        m.mpc_qp_batch(A, B, H, X0[:, :0], 3)
    with pytest.raises(ValueError, match='D and d come together'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=D)
    with pytest.raises(ValueError, match='D and d come together'):
        m.mpc_qp_batch(A, B, H, X0, 3, d=d)
    with pytest.raises(ValueError, match='ndcnt describes the rows of D, which is None'):
        m.mpc_qp_batch(A, B, H, X0, 3, ndcnt=np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match='D \\[nb, p, nd, nx \\+ nu\\]'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=D[..., :5], d=d)
    with pytest.raises(ValueError, match='d \\(2, 3, 2\\) expected'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=D, d=d[..., :1])
    with pytest.raises(ValueError, match='ndcnt int32 \\(2, 3\\) expected'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=D, d=d, ndcnt=np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match='ndcnt in 0 .. nd = 2 expected, got 0 .. 3'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=D, d=d, ndcnt=np.array([[0, 3, 1], [0, 0, 0]], np.int32))
    with pytest.raises(ValueError, match='q \\(2, 3, 6\\) expected'):
        m.mpc_qp_batch(A, B, H, X0, 3, q=np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match='Pf \\(2, 3, 4, 4\\) expected'):
        m.mpc_qp_batch(A, B, H, X0, 3, Pf=np.zeros((2, 3, 6, 6)))
    for bad in (0.0, -1e-8, None, 'x'):
        with pytest.raises(ValueError, match='tol must be a float > 0'):
            m.mpc_qp_batch(A, B, H, X0, 3, tol=bad)
    for bad in (0, 1.5, None):
        with pytest.raises(ValueError, match='max_iter must be an int >= 1'):
            m.mpc_closed_loop_batch(A, B, H, X0, 3, 2, max_iter=bad)
    with pytest.raises(ValueError, match='fp64 arrays expected \\(H has dtype float32\\)'):
        m.mpc_qp_batch(A, B, H.astype(np.float32), X0, 3)
    import torch
    with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(D differs\\)'):
        m.mpc_qp_batch(A, B, H, X0, 3, D=torch.zeros((2, 3, 2, 6), dtype=torch.float64), d=d)
    with pytest.raises(ValueError, match='torch tensors must be float64 tensors of one GPU'):
        m.mpc_qp_batch(*(torch.zeros(x.shape, dtype=torch.float64) for x in (A, B, H, X0)), 3)
    z = np.zeros
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64 \\(got 70\\)'):
        m.mpc_qp_batch(z((1, 2, 40, 40)), z((1, 2, 40, 30)), z((1, 2, 70, 70)), z((1, 1, 40)), 3)
    with pytest.raises(NotImplementedError, match='nx = 40, nu = 24 with room for 200 rows per stage needs \\d+ bytes of LDS \\(limit 163840\\)'):
        m.mpc_qp_batch(z((1, 2, 40, 40)), z((1, 2, 40, 24)), z((1, 2, 64, 64)), z((1, 1, 40)), 3, D=z((1, 2, 200, 64)), d=z((1, 2, 200)))
    with pytest.raises(ValueError, match='mpc_step: x0 must hold nx = 2 entries'):
        m.mpc_step(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(3), 4)
    with pytest.raises(ValueError, match='mpc_closed_loop_sim: D and d come together'):
        m.mpc_closed_loop_sim(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4, 3, D=np.ones((1, 3)))
    with pytest.raises(ValueError, match='mpc_step: D\\[0\\] \\(rows, nx \\+ nu = 3\\)'):
        m.mpc_step(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4, D=np.ones((1, 2)), d=np.ones(1))


def test_the_layout_of_the_kernel_header_is_the_one_restated_in_python():
    from tunempc_amd import mpc_qp as m
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    body = src[src.index('inline MpcQpLds mpc_qp_lds'):src.index('__device__ __forceinline__ double mq_dot')]
    for term in ('l.ld = (n + 1) | 1; l.ldp = nx | 1;', 'l.lv = n + 1 > nd ? n + 1 : nd;', 'l.oP = l.oE + nx * l.ld', 'l.oW = l.oP + nx * l.ldp', 'l.oH = l.oW + nx * l.ld',
                 'l.oD = l.oH + n * l.ld', 'l.oV = l.oD + nd * l.ld', 'l.oR = l.oV + MQ_NVEC * l.lv', '(long long)l.oR + 8',
                 '2LL * (N + 1) * n + 6LL * N * nd + (long long)N * nx + (long long)N * mb * (n + 1)'):
        assert term in body, term
    assert 'constexpr int MQ_NVEC = 24;' in src and 'constexpr int MQ_SLOTS = %d;' % m.SLOTS in src
    consts = re.search(r'MQ_RHO = (\S+), MQ_STEP_BACK = (\S+), MQ_MU_FACTOR = (\S+);', src)
    assert tuple(float(v) for v in consts.groups()) == (mq.RHO, mq.STEP_BACK, mq.MU_FACTOR)
    assert (m.TOL, m.MAX_ITER) == (mq.TOL, mq.MAX_ITER)
    assert m.lds_layout(24, 8, 16)['bytes'] <= 40 * 1024 and m.lds_layout(40, 24, 4)['bytes'] <= 160 * 1024 < m.lds_layout(40, 24, 200)['bytes']
    # the workspace is slots x per-instance bytes: at 512 x 64 instances of the bench stage shape with N = 64 it is 0.1 GB, not the 7 GB of one slot per instance
    per = 8 * m.lds_layout(24, 8, 16)['ws_doubles'](64)
    assert per * m.SLOTS < 2 ** 27 and per * 512 * 64 > 5e9


def test_the_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_batch_host', 'tmpc_mpc_qp_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 31
    assert re.search(r'^#define TMPC_MPC_QP_INFO 8$', header, re.M)
    import tunempc_amd
    assert tunempc_amd.mpc_qp.mpc_qp_batch is not None and tunempc_amd.mpc_qp.mpc_closed_loop_batch is not None


def test_the_library_refuses_by_itself_what_python_refuses():
    """The entries' own checks (a caller of the C ABI does not pass through Python): TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call."""
    from tunempc_amd._lib import load_library
    from tunempc_amd import mpc_qp as m
    lib = load_library()
    d = (C.c_double * 16)()
    i = (C.c_int32 * 4)()
    ok = dict(nb=1, p=2, nx=1, mb=1, nd=0, N=1, ns=1, T=1, k0=0, D=None, dd=None, cnt=None, tol=1e-10, it=60, A=d, U0=d)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    for f, vp in ((lib.tmpc_mpc_qp_batch_host, False), (lib.tmpc_mpc_qp_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)
        I = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: None if x is None else C.cast(x, C.POINTER(C.c_int32)))

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(a['A']), P(d), P(d), None, None, P(a['D']), I(a['cnt']), P(a['dd']), P(d), a['tol'], a['it'], P(a['U0']), P(d), P(d),
                     None, None, None, None, None, None, None, None)
        for kw in (dict(nb=0), dict(p=0), dict(nx=0), dict(mb=0), dict(N=0), dict(ns=0), dict(T=0), dict(nd=-1), dict(k0=2), dict(k0=-1), dict(nd=1), dict(D=d),
                   dict(nd=1, D=d), dict(nd=1, dd=d), dict(cnt=i), dict(tol=0.0), dict(tol=-1.0), dict(tol=float('nan')), dict(it=0), dict(A=None), dict(U0=None)):
            assert call(**kw) == -1, kw
        assert call(nx=40, mb=30) == -2 and b'nx + nu = 64' in lib.tmpc_last_error()
        assert call(nx=40, mb=24, nd=200, D=d, dd=d) == -2
        assert re.search(r'needs (\d+) bytes', lib.tmpc_last_error().decode()).group(1) == str(m.lds_layout(40, 24, 200)['bytes'])
    i[0] = 2
    f = lib.tmpc_mpc_qp_batch_host
    assert f(1, 2, 1, 1, 1, 1, 1, 1, 0, d, d, d, None, None, d, i, d, d, 1e-10, 60, d, d, d, None, None, None, None, None, None, None, None) == -1
    assert b'ndcnt[0][0] = 2 outside 0 .. nd = 1' in lib.tmpc_last_error()
