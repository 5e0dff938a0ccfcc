"""CPU tests of the constraint-to-go recursion: the numpy statement tests/lqr_ctg_reference.py against itself (the recursion (a) against the dense
one-period KKT solve (b), and against tests/lqr_rows_reference.py where the rows fit the inputs), the figures of the AWE golden that bound the GPU test, and
the host-side checks of the state_rows= / rank_tol= arguments of tunempc_amd.lqr (no device needed).

AWE golden (tests/golden/awe_step2_n15.npz: p 40, nx 9, nu 6, 3 + 0..4 rows, max|Pi| = 9.3e7, max|K| = 37.7), tol = 1e-8, measured with numpy:
(a) stops after 3 sweeps on both sides with c_k in 0 .. 2, 12 in all; u_0 of (b) differs from -K_0 x_0 by 2.2e-14 at phase 0 and by up to 1.0e-9 over all 40
phases, 2.7e-11 of max|K|; five further sweeps of (a) move K, Pi, Phi by up to 5.1e-11, 4.2e-12, 2.1e-14 of max(1, max|.|).  The constants below hold
these figures; test_gpu_ctg_lqr.py takes its bound for this golden from them."""
import os
import re

import numpy as np
import pytest

import lqr_ctg_reference as lc
import lqr_rows_reference as lrr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# measured on the AWE golden by the numpy reference alone, relative to max(1, max|.|) of the array (see the module docstring)
AWE_AB_DISAGREEMENT = 2.7e-11        # max over the 40 phases and both sides of |u_0 (b) + K_0 x_0 (a)| / max|K|
AWE_WOBBLE = 5.2e-11                 # largest change of K, Pi or Phi over five sweeps after the stop, both sides
AWE_BOUND = 10.0 * max(AWE_AB_DISAGREEMENT, AWE_WOBBLE)        # what the GPU test allows against the reference and for dK: 5.2e-10
NOISE_MARGIN = 1.5                   # the figures are rounding noise: another BLAS build may move them, not by more than this

SMALL = [lc.case_leftover_row, lc.case_wrap_onto_itself, lc.case_state_only_row, lc.case_duplicated_row, lc.case_accumulating,
         lc.case_rows_within_inputs, lc.case_bench_stage_shape]


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def load_awe():
    g = np.load(os.path.join(GOLDEN, 'awe_step2_n15.npz'))
    d = {k: np.ascontiguousarray(g[k], dtype=np.float64) for k in ('A', 'B', 'H', 'Hc', 'P', 'Hc_tight')}
    d['J'] = np.ascontiguousarray(np.concatenate([g['G'], g['C']], axis=2)); d['ncnt'] = g['ncnt'].astype(np.int32); d['ng'] = g['G'].shape[2]
    return d


def ab_disagreement(A, B, H, J, rows, r, phases):
    """max over the phases of |u_0 of (b) + K_ph x_0| / max(1, max|K|), the period rotated so that it starts at ph."""
    worst = 0.0
    for ph in phases:
        rl = lambda x: np.roll(x, -ph, axis=0)
        Z0, U0 = lc.kkt_first_input(rl(A), rl(B), rl(H), rl(J), rl(rows), r['Pi'][ph], r['Hn'][ph])
        worst = max(worst, np.abs(U0 + r['K'][ph] @ Z0).max())
    return worst / max(1.0, np.abs(r['K']).max())


@pytest.mark.parametrize('case', SMALL, ids=lambda f: f.__name__)
def test_recursion_against_the_dense_one_period_kkt_solve(case):
    A, B, H, J, ncnt = case()[:5]
    for b in range(A.shape[0]):
        r = lc.periodic_lqr(A[b], B[b], H[b], J[b], ncnt[b], tol=lc.TOL)
        if r['infeasible']:
            assert case is lc.case_wrap_onto_itself and b == 0 and r['sweeps'] <= 3
            continue
        assert r['converged'] and r['feas'] <= 1e-10 * max(1.0, np.abs(r['K']).max()), (b, r['sweeps'], r['feas'])
        d = ab_disagreement(A[b], B[b], H[b], J[b], ncnt[b], r, range(A.shape[1]))
        print(case.__name__, b, 'cnt', r['cnt'].tolist(), 'sweeps', r['sweeps'], 'a vs b %.1e' % d, 'feas %.1e' % r['feas'], 'rho %.3g' % r['rho'])
        assert d <= 1e-10, (b, d)


def test_expected_counts_of_the_small_cases():
    c = lambda f, b=0: lc.periodic_lqr(*(x[b] for x in f()[:5]), tol=lc.TOL)['cnt'].tolist()
    assert c(lc.case_leftover_row) == [0, 1, 0]
    assert c(lc.case_state_only_row)[2] >= 1
    assert c(lc.case_accumulating) == [0, 1, 3, 2, 1, 0]
    assert c(lc.case_bench_stage_shape) == [0, 0, 2, 0, 0, 1, 0, 0]
    assert not any(c(lc.case_rows_within_inputs)) and not any(c(lc.case_duplicated_row))


def test_it_is_the_rows_recursion_when_the_rows_fit_the_inputs():
    A, B, H, J, ncnt = lc.case_rows_within_inputs()
    for b in range(A.shape[0]):
        r = lc.periodic_lqr(A[b], B[b], H[b], J[b], ncnt[b], tol=lc.TOL)
        ref = lrr.periodic_lqr(A[b], B[b], H[b], J[b], ncnt[b], tol=lc.TOL)
        e = {k: relmax(r[k], ref[k]) for k in ('K', 'Pi', 'Phi')}
        print(b, e, r['sweeps'], ref['sweeps'])
        assert ref['converged'] and r['converged'] and max(e.values()) <= 1e-13


def test_a_duplicated_row_changes_nothing():
    A, B, H, J, ncnt, ncnt1 = lc.case_duplicated_row()
    J1 = J.copy(); J1[0, 1, 1] = 0.0
    r = lc.periodic_lqr(A[0], B[0], H[0], J[0], ncnt[0], tol=lc.TOL); ref = lrr.periodic_lqr(A[0], B[0], H[0], J1[0], ncnt1[0], tol=lc.TOL)
    assert r['converged'] and relmax(r['K'], ref['K']) <= 1e-12 and relmax(r['Pi'], ref['Pi']) <= 1e-12


def test_awe_golden_certificate_and_the_figures_that_bound_the_gpu_test():
    d = load_awe()
    A, B, J, rows = d['A'][0], d['B'][0], d['J'][0], d['ng'] + d['ncnt'][0]
    rH = lc.periodic_lqr(A, B, d['H'][0], J, rows, Pi0=d['P'][0], tol=1e-8, extra_sweeps=5)
    rC = lc.periodic_lqr(A, B, d['Hc'][0], J, rows, tol=1e-8, extra_sweeps=5)
    rT = lc.periodic_lqr(A, B, d['Hc_tight'][0], J, rows, tol=1e-8)
    ab = max(ab_disagreement(A, B, d[s][0], J, rows, r, range(40)) for s, r in (('H', rH), ('Hc', rC)))
    ab0 = max(ab_disagreement(A, B, d[s][0], J, rows, r, [0]) for s, r in (('H', rH), ('Hc', rC)))
    wob = max(max(r['wobble'].values()) for r in (rH, rC))
    dK = np.abs(rH['K'] - rC['K']).max(); dKt = np.abs(rH['K'] - rT['K']).max()
    print('sweeps', rH['sweeps'], rC['sweeps'], 'cnt sum', rH['cnt'].sum(), 'max', rH['cnt'].max(), 'max|K| %.1f max|Pi| %.2e' % (np.abs(rC['K']).max(), np.abs(rC['Pi']).max()))
    print('a vs b: phase 0 %.2e, all phases %.2e; wobble H %s Hc %s' % (ab0, ab, rH['wobble'], rC['wobble']))
    print('dK %.2e (tight %.2e)  subspace diff %.1e  feas %.1e %.1e  rho %.3g %.3g' % (dK, dKt, np.abs(rH['Pz'] - rC['Pz']).max(), rH['feas'], rC['feas'], rH['rho'], rC['rho']))
    assert rH['converged'] and rC['converged'] and rT['converged'] and rH['sweeps'] <= 5 and rC['sweeps'] <= 5
    assert (rH['cnt'] == rC['cnt']).all() and rH['cnt'].sum() == 12 and rH['cnt'].max() == 2
    assert np.abs(rH['Pz'] - rC['Pz']).max() <= 1e-12
    assert rH['feas'] <= 1e-10 and rC['feas'] <= 1e-10 and rH['rho'] < 1.0 and rC['rho'] < 1.0
    assert ab <= NOISE_MARGIN * AWE_AB_DISAGREEMENT and wob <= NOISE_MARGIN * AWE_WOBBLE, (ab, wob)
    kmax = np.abs(rC['K']).max()
    assert dK / kmax <= AWE_BOUND and dKt / kmax <= AWE_BOUND


# ----------------------------------------------------------------------------- the C ABI and the host-side argument checks (no device needed)
def test_the_ctg_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_periodic_lqr_ctg_batch_host', 'tmpc_periodic_lqr_ctg_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 21


def _batch(nb=2, p=3, nx=4, mb=2):
    return np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, mb)), np.tile(np.eye(nx + mb), (nb, p, 1, 1))


def test_state_rows_needs_rows_and_a_sane_rank_tol():
    from tunempc_amd import lqr
    A, B, H = _batch()
    J = np.zeros((2, 3, 2, 6))
    with pytest.raises(ValueError, match='state_rows=True is the recursion for the rows of J, which is None'):
        lqr.periodic_lqr_batch(A, B, H, state_rows=True)
    with pytest.raises(ValueError, match='state_rows=True is the recursion for the rows of J, which is None'):
        lqr.feedback_equivalence_batch(A, B, H, H, state_rows=True)
    for bad in (0.0, -1e-9, 1.0, float('nan'), 'tight', None, True):
        with pytest.raises(ValueError, match='0 < rank_tol < 1 expected'):
            lqr.periodic_lqr_batch(A, B, H, J=J, state_rows=True, rank_tol=bad)
    args = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)))
    with pytest.raises(ValueError, match='state_rows=True is the recursion for the rows G / C, which are None'):
        lqr.periodic_lqr(*args, state_rows=True)
    with pytest.raises(ValueError, match='state_rows=True is the recursion for the rows G / C, which are None'):
        lqr.feedback_equivalence(*args, [np.zeros((3, 3))], state_rows=True)
    assert lqr.STATUS_NAMES[5] == 'NoFeasibleSubspace' and lqr.STATUS_NAMES[4] == 'RowsExceedInputs'


def test_ctg_refusals_carry_the_library_message():
    """A shape beyond the 160 KB of LDS of the wider layout and nr < ng are refused by the library before it touches a device."""
    from tunempc_amd import lqr
    A, B, H = _batch(1, 2, 32, 32)
    with pytest.raises(NotImplementedError, match='nx = 32, nu = 32 with room for 8 rows per stage and a constraint-to-go needs 216064 bytes of LDS \\(limit 163840\\)'):
        lqr.periodic_lqr_batch(A, B, H, J=np.zeros((1, 2, 8, 64)), state_rows=True)
    A, B, H = _batch()
    with pytest.raises(ValueError, match='0 <= ng <= nr, the row capacity per stage.*ng = 3, nr = 2'):
        lqr.periodic_lqr_batch(A, B, H, J=np.zeros((2, 3, 2, 6)), ng=3, state_rows=True)


def test_the_ctg_lds_layout():
    """The layout formula of csrc/tmpc_lqr_ctg.h restated: 61 KB at the bench stage shape with room for 10 rows; every n <= 32 fits with any nr <= 66, every n <= 48 with any nr <= 15."""
    def total(nx, mb, nr):
        n = nx + mb
        nbd, ms = min(mb, nr + nx), max(nr + nx, mb)
        ld, ldp, ldc = (n + nbd) | 1, nx | 1, n | 1
        return (nx * ld + nx * ldp + max(nx, mb + nbd) * ld + (n + nbd) * ld + 2 * ms * ldc + 2 * nx * ldp + 16) * 8
    assert total(24, 8, 10) == 61344 and total(9, 6, 7) < 16 * 1024
    assert total(32, 32, 8) == 216064
    assert max(total(nx, n - nx, 66) for n in range(2, 33) for nx in range(1, n)) <= 160 * 1024
    assert max(total(nx, n - nx, 15) for n in range(33, 49) for nx in range(1, n)) <= 160 * 1024
