"""GPU tests of what the entries of the local gain (tmpc_mpc_qp_gain_batch_host / _device, tunempc_amd.mpc_qp.mpc_qp_gain_batch) promise beyond the values:
bit-identity of the two entries, of an instance alone against the same instance among others, and of the call without its optional outputs; a failed
instance (NaN in its solution: status 3) or an active set that leaves no direction (status 5) does not disturb its neighbours; a shape beyond the LDS layout
is refused before the device; mpc_step_gain is the batch call on one model."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_reference as mq  # noqa: E402
import mpc_qp_eq_reference as eqr  # noqa: E402
import mpc_qp_quad_reference as mqq  # noqa: E402
import mpc_qp_gain_reference as gr  # noqa: E402
from test_gpu_mpc_qp_gain import solve, gain, to_host, to_dev  # noqa: E402

CORE = ('K0', 'Pi0', 'Hn0', 'cnt0', 'info', 'cls', 'strict', 'status', 'feas', 'nactive')
ALL = CORE + ('Kall', 'cntall', 'dX', 'dU')


def same(a, b, keys, idx=None):
    for k in keys:
        x, y = (a[k], b[k]) if idx is None else (a[k][idx[0]], b[k][idx[1]])
        np.testing.assert_array_equal(x, y, err_msg=k)


def solved_host(bt):
    """The solution of the device entry as numpy arrays: one solution for both entries of the gain."""
    return {k: v for k, v in to_host(solve('device', bt)).items() if k in ('X', 'U', 'lam', 'eps')}


def dev_sol(sol):
    return {k: to_dev(v) for k, v in sol.items()}


def _batches():
    i = mqq.infeasible_instance(50.0, 500.0)
    return [('state box', gr.batch_of_case(gr.case_state_box())), ('mixed small', gr.batch_of_case(mq.case_mixed_small())),
            ('rows and Tx', eqr.batch_of(eqr.case_rows_mixed_small())), ('L1 + L2', dict(mqq.batch_of([i]), J=None, r=None, necnt=None, terminal=None))]


def test_host_and_device_entry_agree_bit_for_bit():
    for name, bt in _batches():
        sol = solved_host(bt)
        h = gain('host', bt, sol, return_all=True)
        d = to_host(gain('device', bt, dev_sol(sol), return_all=True))
        assert not h['status'].any(), (name, h['status'])
        same(h, d, ALL)
        act = np.ascontiguousarray(np.roll(h['cls'], 1, axis=2))             # some other active set, through cls_in
        ha = gain('host', bt, sol, active=act)
        da = to_host(gain('device', bt, dev_sol(sol), active=to_dev(act)))
        same(ha, da, CORE)


def test_an_instance_does_not_depend_on_ns_or_on_its_neighbours():
    bt = gr.batch_of_case(gr.case_state_box())
    sol = solved_host(bt)
    full = gain('host', bt, sol, return_all=True)
    for ns in (1, 2, 3):
        for first in (0, 1):
            sl = slice(first, first + ns)
            part = gain('host', dict(bt, X0=bt['X0'][:, sl]), {k: np.ascontiguousarray(v[:, sl]) for k, v in sol.items()}, return_all=True)
            for k in ALL:
                np.testing.assert_array_equal(part[k], full[k][:, sl], err_msg='%s ns=%d first=%d' % (k, ns, first))


def test_absent_optional_outputs_change_nothing():
    for name, bt in _batches():
        sol = dev_sol(solved_host(bt))
        same(to_host(gain('device', bt, sol)), to_host(gain('device', bt, sol, return_all=True)), CORE)


def test_a_failed_instance_ends_with_status_3_and_leaves_the_rest_alone():
    bt = gr.batch_of_case(gr.case_state_box())
    sol = solved_host(bt)
    clean = gain('host', bt, sol, return_all=True)
    for key, where in (('X', (0, 1, 2, 0)), ('lam', (0, 1, 3, 1)), ('U', (0, 1, 0, 0))):
        bad = {k: v.copy() for k, v in sol.items()}
        bad[key][where] = np.nan
        for entry in ('host', 'device'):
            o = to_host(gain(entry, bt, dev_sol(bad) if entry == 'device' else bad, return_all=True))
            assert o['status'][0, 1] == 3 and o['cnt0'][0, 1] == 0
            for k in ('K0', 'Pi0', 'strict', 'Kall', 'dX', 'dU'):
                assert np.isnan(o[k][0, 1]).all(), k
            assert not o['Hn0'][0, 1].any() and (o['cls'][0, 1] == -1).all() and (o['cntall'][0, 1] == -1).all()
            for s in (0, 2, 3):
                same(o, clean, ALL, ((0, s), (0, s)))
    # a whole failed solve, as mpc_qp_batch returns it: every array NaN
    bad = {k: v.copy() for k, v in sol.items()}
    for v in bad.values():
        v[0, 2] = np.nan
    o = gain('host', bt, bad)
    assert o['status'][0].tolist() == [0, 0, 3, 0]
    same(o, clean, CORE, ((0, 3), (0, 3)))


def test_an_active_set_that_leaves_no_direction_ends_with_status_5():
    """Three independent rows on the state alone, held as equalities at stage 1 of instance 1: x_1 = 0 is all that is left there."""
    c = mq.case_box_nu2()
    bt = gr.batch_of_case(c)
    nb, p, nx, _ = bt['A'].shape
    n = bt['H'].shape[2]
    D = np.zeros((nb, p, 3, n)); D[:, :, :, :nx] = np.eye(nx)
    bt.update(D=D, d=np.full((nb, p, 3), 50.0), ndcnt=None)
    sol = solved_host(bt)
    ns, N = bt['X0'].shape[1], bt['N']
    free = np.zeros((nb, ns, N, 3), np.int32)
    clean = gain('host', bt, sol, active=free, return_all=True)
    act = free.copy(); act[0, 1, 1] = 1
    for entry in ('host', 'device'):
        o = to_host(gain(entry, bt, dev_sol(sol) if entry == 'device' else sol, active=to_dev(act) if entry == 'device' else act, return_all=True))
        assert o['status'][0].tolist() == [0, 5, 0, 0] and o['cnt0'][0, 1] == nx
        assert np.isnan(o['K0'][0, 1]).all() and np.isnan(o['Pi0'][0, 1]).all() and np.isnan(o['strict'][0, 1]) and np.isnan(o['Kall'][0, 1, :2]).all()
        assert np.isfinite(o['Kall'][0, 1, 2:]).all() and o['cntall'][0, 1].tolist() == [-1, -1, 0, 0] and (o['cls'][0, 1, :2] == -1).all()
        for s in (0, 2, 3):
            same(o, clean, ALL, ((0, s), (0, s)))
    # two of the three rows leave one direction: status 0, cnt = 2 at that stage
    act = free.copy(); act[0, 1, 1, :2] = 1
    o = gain('host', bt, sol, active=act, return_all=True)
    assert o['status'][0, 1] == 0 and o['cntall'][0, 1, 1] == 2


def test_a_layout_beyond_160_kb_is_refused_before_the_device():
    from tunempc_amd import mpc_qp as m
    nb, ns, p, nx, nu, nd, N = 1, 1, 2, 20, 4, 330, 3
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device='cuda')
    sol = dict(X=z(nb, ns, N + 1, nx), U=z(nb, ns, N, nu), lam=z(nb, ns, N, nd))
    assert m.lds_layout(nx, nu, nd)['bytes'] <= m.LDS_BYTES < m.gain_lds_bytes(nx, nu, nd)
    with pytest.raises(NotImplementedError, match='mpc_qp_gain_batch: nx = 20, nu = 4 with room for 0 \\+ 330 rows per stage and a constraint-to-go needs \\d+ bytes'):
        m.mpc_qp_gain_batch(z(nb, p, nx, nx), z(nb, p, nx, nu), z(nb, p, nx + nu, nx + nu), sol, N, D=z(nb, p, nd, nx + nu), d=z(nb, p, nd))


def test_mpc_step_gain_is_the_batch_call_on_one_model():
    from tunempc_amd import mpc_qp as m
    c = mq.case_single_phase()
    nx = c['A'].shape[2]
    A, B, H = c['A'][0, 0], c['B'][0, 0], c['H'][0, 0]
    Q, R, Nc = H[:nx, :nx], H[nx:, nx:], H[:nx, nx:]
    bt = gr.batch_of_case(c)
    sol = solved_host(bt)
    g = gain('host', bt, sol)
    for s in range(bt['X0'].shape[1]):
        u0, X, U, lam, info = m.mpc_step(A, B, Q, R, Nc, c['X0'][0, s], c['N'], c['k0'], D=c['D'][0, 0], d=c['d'][0, 0], Pf=c['Pf'][0, 0])
        np.testing.assert_array_equal(X, sol['X'][0, s])
        K0, gi = m.mpc_step_gain(A, B, Q, R, Nc, dict(X=X, U=U, lam=lam), c['N'], c['k0'], D=c['D'][0, 0], d=c['d'][0, 0], Pf=c['Pf'][0, 0])
        np.testing.assert_array_equal(K0, g['K0'][0, s])
        assert gi['status'] == 0 and gi['cnt0'] == g['cnt0'][0, s] and np.array_equal(gi['cls'], g['cls'][0, s]) and gi['strict'] == g['strict'][0, s]
    with pytest.raises(RuntimeError, match='mpc_step_gain: the pass ended with status 3'):
        m.mpc_step_gain(A, B, Q, R, Nc, dict(X=np.full_like(X, np.nan), U=U, lam=lam), c['N'], c['k0'], D=c['D'][0, 0], d=c['d'][0, 0], Pf=c['Pf'][0, 0])


def test_a_zero_penalty_beside_a_zero_penalty2_is_a_row_that_cannot_be_active():
    """The Python layer refuses c = 0 with Z = 0; the C entry takes it as class 0 with s = g: nothing is divided by zero, the gain is the one with every row free."""
    from tunempc_amd import _lib
    bt = gr.batch_of_case(mq.case_box_nu2())
    sol = solved_host(bt)
    nb, ns = bt['X0'].shape[:2]
    z = np.zeros(bt['d'].shape)
    c = lambda x: np.ascontiguousarray(x)
    o = _lib.mpc_qp_gain_batch_host(c(bt['A']), c(bt['B']), c(bt['H']), c(bt['Pf']), c(bt['D']), None, c(bt['d']), z, z.copy(), None, None, 0, None, sol['X'], sol['U'],
                                    sol['lam'], np.zeros_like(sol['lam']), None, bt['N'], bt['k0'], 1e-9, False)
    free = gain('host', bt, sol, active=np.zeros((nb, ns, bt['N'], bt['D'].shape[2]), np.int32))
    assert not o['cls'].any() and np.isfinite(o['strict']).all() and not o['info'][..., 0].any()
    np.testing.assert_array_equal(o['K0'], free['K0'])
