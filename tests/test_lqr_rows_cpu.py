"""CPU tests of the periodic LQ recursion with rows (tests/lqr_rows_reference.py) and of the host-side checks of tunempc_amd.lqr for the rows arguments.

The data are Step 2 solutions of oracle/cpu_ipm at a shape it solves in seconds (p 8, nx 6, nu 4, one row of G_k and 0..2 rows of C_k, rho = 1e-3: the
multipliers are active, 1.1 ... 1.9).  Checked: the two forms of the stage solve agree; the theorem -- with the rows held as equalities the LQ problems on H
(from Pi0 = P) and on Hc (from zero) have the same gains and Pi(H) = Pi(Hc) + P, while the unconstrained recursion on the same data gives gains that differ
by 0.2; and a problem without rows is the plain recursion, exactly."""
import os
import re

import numpy as np
import pytest

import cpu_ipm
import lqr_reference as lr
import lqr_rows_reference as lrr
from tunempc_amd.synthetic import gen_batch

THREADS = max(1, min(8, len(os.sched_getaffinity(0))))
P, NX, MB, NG, NC, NB = 8, 6, 4, 1, 2, 3


@pytest.fixture(scope='module')
def step2():
    A, B, H = gen_batch(5, NB, P, NX, MB)
    J, ncnt = lrr.gen_rows(6, NB, P, NX + MB, NG, NC)
    res = cpu_ipm.convexify_con_batch(A, B, H, J, ng=NG, ncnt=ncnt, rho=1e-3, threads=THREADS)
    assert (res['status'] == 0).all(), res['status']
    print('multipliers max', res['FgF'].reshape(NB, -1).max(axis=1))
    return dict(A=A, B=B, H=H, J=J, rows=NG + ncnt, Hc=res['Hc'], Pm=res['P'], F=res['FgF'])


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_nullspace_form_equals_kkt_form(step2):
    """K, Pi (and Lam) of the two forms of the stage solve, run to convergence independently, to 1e-9 relative on every member and on both sides."""
    d = step2
    for b in range(NB):
        for side, Pi0 in (('H', d['Pm'][b]), ('Hc', None)):
            a = lrr.periodic_lqr(d['A'][b], d['B'][b], d[side][b], d['J'][b], d['rows'][b], Pi0=Pi0)
            k = lrr.periodic_lqr(d['A'][b], d['B'][b], d[side][b], d['J'][b], d['rows'][b], Pi0=Pi0, method='kkt')
            e = {key: relmax(a[key], k[key]) for key in ('K', 'Pi', 'Lam')}
            print(b, side, 'sweeps', a['sweeps'], k['sweeps'], e, 'max|Pi|', np.abs(a['Pi']).max())
            assert a['converged'] and k['converged']
            assert e['K'] <= 1e-9 and e['Pi'] <= 1e-9 and e['Lam'] <= 1e-9


def test_constrained_feedback_equivalence_and_the_unconstrained_contrast(step2):
    d = step2
    for b in range(NB):
        A, B, H, Hc, Pm, J, rows = (d[k][b] for k in ('A', 'B', 'H', 'Hc', 'Pm', 'J', 'rows'))
        assert d['F'][b].max() > 1e-2                                            # the multipliers are active: the contrast is there to be seen
        rH = lrr.periodic_lqr(A, B, H, J, rows, Pi0=Pm)
        rC = lrr.periodic_lqr(A, B, Hc, J, rows)
        dK = np.abs(rH['K'] - rC['K']).max()
        dPi = np.abs(rH['Pi'] - rC['Pi'] - Pm).max()
        uH = lr.periodic_lqr(A, B, H, Pi0=Pm); uC = lr.periodic_lqr(A, B, Hc)
        dKu = np.abs(uH['K'] - uC['K']).max()
        print(b, 'multiplier max %.2f  dK rows %.1e  unconstrained %.2e  dPi %.1e  feas %.1e %.1e  rho %.3g %.3g  sweeps %d %d' % (
            d['F'][b].max(), dK, dKu, dPi, rH['feas'], rC['feas'], rH['rho'], rC['rho'], rH['sweeps'], rC['sweeps']))
        assert rH['converged'] and rC['converged'] and uH['converged'] and uC['converged']
        assert dK <= 1e-8
        assert dPi <= 1e-8 * max(np.abs(rH['Pi']).max(), np.abs(rC['Pi']).max())
        for r in (rH, rC):
            assert r['feas'] <= 1e-9 * max(1.0, np.abs(r['K']).max())
            assert r['rho'] < 1.0
        assert dKu > 1e-3


def test_without_rows_it_is_the_plain_recursion_exactly(step2):
    d = step2
    for b in range(NB):
        ref = lr.periodic_lqr(d['A'][b], d['B'][b], d['Hc'][b])
        for J, rows in ((None, None), (d['J'][b], np.zeros(P, int))):
            for method in ('nullspace', 'kkt'):
                r = lrr.periodic_lqr(d['A'][b], d['B'][b], d['Hc'][b], J, rows, method=method)
                assert r['sweeps'] == ref['sweeps']
                for k in ('K', 'Pi', 'Phi'):
                    np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def test_an_input_constrained_stage_has_the_gain_the_rows_dictate():
    """r = nu with a square invertible Ju: the rows alone fix K = Ju^-1 Jx, whatever the cost -- both forms."""
    rng = np.random.default_rng(3)
    nx, mb = 3, 2
    Hb = rng.standard_normal((5, 5)); Hb = Hb + Hb.T
    Jk = rng.standard_normal((mb, nx + mb))
    want = np.linalg.solve(Jk[:, nx:], Jk[:, :nx])
    for method in ('nullspace', 'kkt'):
        K, Lam, Pk = lrr.stage(Hb, Jk, nx, method)
        T = np.concatenate([np.eye(nx), -want])
        assert np.abs(K - want).max() <= 1e-12 and np.abs(Pk - T.T @ Hb @ T).max() <= 1e-11
        assert np.abs(Hb[nx:, nx:] @ K + Jk[:, nx:].T @ Lam - Hb[nx:, :nx]).max() <= 1e-11


# ----------------------------------------------------------------------------- the C ABI and the host-side argument checks (no device needed)
def test_the_rows_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_periodic_lqr_rows_batch_host', 'tmpc_periodic_lqr_rows_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 19


def _batch(nb=2, p=3, nx=4, mb=2):
    return np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, mb)), np.tile(np.eye(nx + mb), (nb, p, 1, 1))


def test_rows_shape_and_dtype_errors_are_raised_before_any_device_call():
    from tunempc_amd import lqr
    A, B, H = _batch()
    J = np.zeros((2, 3, 2, 6)); ncnt = np.zeros((2, 3), np.int32)
    with pytest.raises(ValueError, match='J \\[nb, p, nr, nx \\+ nu\\]'):
        lqr.periodic_lqr_batch(A, B, H, J=J[:, :, :, :5])
    with pytest.raises(ValueError, match='J \\[nb, p, nr, nx \\+ nu\\]'):
        lqr.periodic_lqr_batch(A, B, H, J=J[0])
    with pytest.raises(ValueError, match='fp64'):
        lqr.periodic_lqr_batch(A, B, H, J=J.astype(np.float32))
    with pytest.raises(ValueError, match='int32'):
        lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt.astype(np.int64), ng=1)
    with pytest.raises(ValueError, match='ncnt \\[nb, p\\]'):
        lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt[:1], ng=1)
    with pytest.raises(ValueError, match='0 <= ncnt <= J.shape\\[2\\] - ng = 1'):
        lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt + 2, ng=1)
    with pytest.raises(ValueError, match='0 <= ncnt'):
        lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt - 1, ng=1)
    with pytest.raises(ValueError, match='ng'):
        lqr.periodic_lqr_batch(A, B, H, J=J, ng=-1)
    with pytest.raises(ValueError, match='J, which is None'):
        lqr.periodic_lqr_batch(A, B, H, ncnt=ncnt)
    with pytest.raises(ValueError, match='must be a numpy array'):
        lqr.periodic_lqr_batch(A, B, H, J=[[0.0]])
    with pytest.raises(ValueError, match='J \\[nb, p, nr, nx \\+ nu\\]'):
        lqr.feedback_equivalence_batch(A, B, H, H, J=J[:1])
    with pytest.raises(ValueError, match='nx \\+ nu = 3 columns'):
        lqr.periodic_lqr(np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), G=np.ones((1, 4)))


def test_rows_refusals_carry_the_library_message():
    """nr < ng and a shape beyond the 160 KB of LDS are refused by the library before it touches a device."""
    from tunempc_amd import lqr
    A, B, H = _batch()
    with pytest.raises(ValueError, match='0 <= ng <= nr, the row capacity per stage.*ng = 3, nr = 2'):
        lqr.periodic_lqr_batch(A, B, H, J=np.zeros((2, 3, 2, 6)), ng=3)
    A, B, H = _batch(1, 2, 32, 32)
    with pytest.raises(NotImplementedError, match='nx = 32, nu = 32 with room for 40 rows per stage needs 183296 bytes of LDS \\(limit 163840\\)'):
        lqr.periodic_lqr_batch(A, B, H, J=np.zeros((1, 2, 40, 64)))
    with pytest.raises(NotImplementedError, match='nx \\+ nu = 64 \\(got 65\\)'):
        lqr.periodic_lqr_batch(*_batch(1, 2, 50, 15), J=np.zeros((1, 2, 1, 65)))


def test_the_lds_layout_limits_stated_in_the_header():
    """The limits the header and DESIGN.md state, from the layout formula of csrc/tmpc_lqr_rows.h restated here: n <= 32 fits with any nr <= 66, 32 < n <= 64
    with any nr <= 15; nx = nu = nr = 32 fits."""
    def total(nx, mb, nr):
        n, nk = nx + mb, mb + nr
        ld, ldp = (n + nr) | 1, nx | 1
        return (nx * ld + nx * ldp + max(nx, nk) * ld + (n + nr) * ld + 16) * 8
    assert max(total(nx, n - nx, 66) for n in range(2, 33) for nx in range(1, n)) <= 160 * 1024
    assert max(total(nx, n - nx, 15) for n in range(33, 65) for nx in range(1, n)) <= 160 * 1024
    assert total(32, 32, 16) > 0 and total(32, 32, 32) <= 160 * 1024 < total(32, 32, 40) == 183296
    assert total(24, 8, 5) == 30088 and total(24, 8, 0) == 26048
