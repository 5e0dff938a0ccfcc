"""Kernel-level check of the linear system of one interior-point iteration: k_stage_pre (inverses, residuals, Kronecker factors), k_schur<0/1> and its
global-scratch form (diagonal and coupling blocks), k_stage_rhs and k_gather (right-hand side and border columns), and the generic kb_stage_* forms -- at iterates
the SOLVER reached: the call runs iterations 1 .. K-1 as always and stops with the assembled, unfactored system of iteration K in the workspace
(TMPC_DEBUG_FLAG_STOP_ASSEMBLED + tmpc_debug_set_stop_iteration, include/tunempc_hip_debug.h).

Every layer is compared with tests/schur_reference.py (numpy, np.longdouble) evaluated on that layer's OWN device inputs, so every tolerance is a rounding bound:
|device - reference| <= 4 gamma_m * bound, entrywise, with eps = 2^-53, gamma_m = m eps / (1 - m eps), m the number of nested fp64 operations of an entry (written
at each assert), `bound` the same formula on the absolute values of the inputs, and the factor 4 for FMA contraction and the order of summation.

tmpc_debug_get_array reads lane 0 only: the handle is created with chunk = batch size and lanes = 1 (tmpc_create_ex), so the whole batch is one chunk on that lane
and problem b sits at index b of every array.

The rows of the G / C multipliers (k_phi_pre, k_aug_fill, k_phi_rhs, k_aug_gather) are in tests/test_gpu_phi_kernels.py, the rows of Step 3
(tmpc_t3.h) in tests/test_gpu_t3_kernels.py.  Not covered here: the double-double assembly of the tight mode (k_dd_aug_fill with it), and the one-wave schur_body inside the persistent kernel
(test_gpu_batch_parity.py::test_persistent_small_kernel_parity).  Centering iterates (three-column pass 2, chord steps) and everything after the block solve
-- pass-2 right-hand side, border solve, directions, step lengths, update -- are in tests/test_gpu_step_kernels.py."""
import numpy as np
import pytest

import schur_reference as sr
from schur_assembly_cases import CASES, SMALL_CASES, make_problem, solved_members

pytestmark = pytest.mark.gpu

FLAG_STOP_ASSEMBLED, FLAG_GENERIC_STAGE = 8, 64
P_TAU, P_ALPHA, P_MU, P_SIGMU = 0, 1, 4, 6      # csrc/tmpc_common.h
PS, TRACE_LEN, TRACE_W = 48, 80, 10
# which-codes of tmpc_debug_get_array (include/tunempc_hip_debug.h)
CODES = dict(Ddiag=2, D=3, O=5, W3=7, U=8, X1=9, X2=10, S1=11, S2=12, P=13, V=14, Hb=15, S1i=16, S2i=17, Rd1=18, Rd2=19, T1=20, T2=21, KF=22, adjV=23, adjE=24,
             prob=26, trace=27)

# the five small shapes once more with the generic per-stage kernels (kb_stage_pre / kb_stage_rhs at n <= 32, same inputs)
PARAMS = [(s, k, False) for s, k in CASES] + [(s, k, True) for s, k in CASES if s in SMALL_CASES]


def _id(prm):
    (nb, p, nx, mb), k, generic = prm
    return f'nb{nb}-p{p}-nx{nx}-mb{mb}-K{k}' + ('-generic' if generic else '')


@pytest.fixture(scope='module', params=PARAMS, ids=_id)
def case(request):
    """one device call per (shape, K, stage-kernel form): everything the assembly kernels read and wrote, per problem"""
    from tunempc_amd._lib import HipConvexifier, cr_schedule
    shape, K, generic = request.param
    nb, p, nx, mb = shape
    n = nx + mb; d = nx * (nx + 1) // 2; dp = (d + 15) // 16 * 16
    A, B, H = make_problem(shape)
    h = HipConvexifier(p, nx, mb, chunk=nb, lanes=1, flags=FLAG_STOP_ASSEMBLED | (FLAG_GENERIC_STAGE if generic else 0))
    assert h.chunk == nb
    h.debug_set_stop_iteration(K)
    h.convexify_batch(A, B, H)
    shp = dict(Ddiag=(p, dp), D=(p, dp, dp), O=(p, dp, dp), W3=(p, dp, 3), U=(p, dp, 2), P=(p, nx, nx), V=(p, nx, n), KF=(p, 12, nx, nx),
               adjV=(p, 3, nx, nx), adjE=(p, 3, nx, nx), prob=(PS,), trace=(TRACE_LEN, TRACE_W))
    c = dict(shape=shape, K=K, n=n, d=d, dp=dp, solved=solved_members(shape), orient=cr_schedule(p)['orient'])
    for name, code in CODES.items():
        s = (nb,) + shp.get(name, (p, n, n))
        c[name] = h.debug_array(code, 0, int(np.prod(s))).reshape(s)
    h.close()
    return c


def _inside(got, ref, bound, m, what):
    """|got - ref| <= 4 gamma_m bound, entrywise; the message names the worst entry"""
    err = np.abs(np.asarray(got, sr.LD) - ref)
    lim = 4 * sr.gamma(m) * bound
    bad = err > lim
    if np.any(bad):
        i = np.unravel_index(np.argmax(np.where(bad, err - lim, -np.inf)), err.shape)
        pytest.fail(f'{what}: {int(bad.sum())} of {err.size} entries outside 4 gamma_{m} * bound; worst at {i}: device {float(np.asarray(got)[i])!r} '
                    f'reference {float(ref[i])!r} error {float(err[i]):.3e} limit {float(lim[i]):.3e}')


def test_stopped_at_iteration_K_in_the_main_phase(case):
    """iterations 1 .. K-1 were taken in the main phase without a frozen pivot (so I_REG = 0: no lift of the Schur diagonal), the call stopped inside iteration K
    (k_ctrl_a ran, k_ctrl_c -- which writes the row of the trace -- did not), still in the main phase; for K >= 2 the iterate has left the starting point"""
    nb, p, nx, mb = case['shape']
    K, n = case['K'], case['n']
    for b in range(nb):
        tr, pr = case['trace'][b], case['prob'][b]
        if b not in case['solved']:
            assert not tr.any()                                    # left at the pre-check: never iterated
            continue
        for i in range(1, K):
            row = tr[i - 1]
            assert row[0] == i and row[1] == 0.0 and row[9] == 0.0, (i, row)        # iteration, phase MAIN (x.25 = chord step), shifts + failed stage pivots
            assert row[6] > 0.0 and row[7] > 0.0, (i, row)                           # both step lengths: the step was taken, not repeated
        assert not tr[K - 1:].any()                                                   # row K is written by the k_ctrl_c the call stopped short of
        assert pr[P_MU] > 0.0 and pr[P_SIGMU] == 0.0                                  # k_ctrl_a of iteration K: main phase (centering sets sigma mu = mu_t > 0)
        x0I = np.eye(n) / (p * n)
        X1, X2, S1 = case['X1'][b], case['X2'][b], case['S1'][b]
        if K == 1:
            assert np.array_equal(X1, np.broadcast_to(x0I, X1.shape)) and np.array_equal(X1, X2) and np.array_equal(S1, np.broadcast_to(np.eye(n), S1.shape))
        else:
            assert np.linalg.norm(X1 - x0I) > 1e-2 * np.linalg.norm(X1), 'X1 still at the starting point'
            assert np.linalg.norm(S1 - np.eye(n)) > 1e-2 * np.linalg.norm(S1), 'S1 still at the starting point'
            assert np.linalg.norm(X1 - X2) > 1e-2 * np.linalg.norm(X1), 'X1 == X2'


def test_inverses(case):
    """S_r^-1 of k_stage_pre / kb_stage_pre (Cholesky, triangular inverse, L^-T L^-1): ||S_r S_ri - I||_max <= 4 gamma_{3n} cond_2(S_r); m = 3n: n terms in each of
    the factorisation, the triangular inverse and the product"""
    n = case['n']
    for b in case['solved']:
        for r in (1, 2):
            S, Si = case[f'S{r}'][b], case[f'S{r}i'][b]
            res = np.abs(sr.inverse_residual(S, Si)).max(axis=(1, 2))
            lim = 4 * sr.gamma(3 * n) * np.linalg.cond(S)
            assert np.all(res <= lim), (b, r, res, lim)
            assert np.array_equal(Si, np.swapaxes(Si, 1, 2))       # stored symmetrised


def test_kronecker_factors(case):
    """all 12 slots of KF against kron_factors(X_r, device S_r^-1, V); m = 2n: V X V' is two nested sums of n products (the copies XXX, SIXX are exact)"""
    nb, p, nx, mb = case['shape']
    n = case['n']
    for b in case['solved']:
        for r in (1, 2):
            ref, bound = sr.kron_factors(case[f'X{r}'][b], case[f'S{r}i'][b], case['V'][b], nx)
            _inside(case['KF'][b][:, 6 * (r - 1):6 * r], ref, bound, 2 * n, f'problem {b} KF of LMI {r} [stage, slot, i, j]')


def test_schur_blocks(case):
    """the lower triangle of D_k and the edge slot O[k] against schur_blocks(device KF); m = 32: an entry of D is 16 products and their sums, of C 8"""
    nb, p, nx, mb = case['shape']
    d = case['d']
    low = np.tril(np.ones((d, d), bool))
    for b in case['solved']:
        D, C, Db, Cb = sr.schur_blocks(case['KF'][b], p, nx)
        got = case['D'][b][:, :d, :d]
        _inside(np.where(low, got, 0.0), np.where(low, D, 0), Db, 32, f'problem {b} D [stage, row, col]')
        # edge slot k: orientation 0 = stored as C_k' = T[P_{k+1}, P_k], 1 = as C_k = T[P_k, P_{k+1}]
        Cgot = np.stack([case['O'][b][k, :d, :d].T if case['orient'][k] == 0 else case['O'][b][k, :d, :d] for k in range(p)])
        _inside(Cgot, C, Cb, 32, f'problem {b} C [stage, (ab) of P_k, (cd) of P_k+1]')


def test_schur_padding_and_diagonal(case):
    """Ddiag is the diagonal of D bit for bit; rows and columns beyond d: identity in the lower triangle of D (the upper one is never written), ones in Ddiag,
    zeros in O -- all exact"""
    nb, p, nx, mb = case['shape']
    d, dp = case['d'], case['dp']
    for b in case['solved']:
        D, O, Dd = case['D'][b], case['O'][b], case['Ddiag'][b]
        for k in range(p):
            assert np.array_equal(Dd[k, :d], np.diagonal(D[k])[:d])
            assert np.array_equal(np.tril(D[k])[d:, :], np.eye(dp)[d:, :])
            assert np.array_equal(Dd[k, d:], np.ones(dp - d))
            assert not O[k, d:, :].any() and not O[k, :, d:].any()


def test_right_hand_sides(case):
    """k_stage_pre's residuals, k_stage_rhs's T_r, and the three pass-1 columns that k_gather leaves in W3 and U, each from the device values of the layer before"""
    nb, p, nx, mb = case['shape']
    n, d = case['n'], case['d']
    ia, ib = sr.tri_idx(nx)
    wgt = np.where(ia == ib, 1, 2).astype(sr.LD)
    for b in case['solved']:
        g = {k: case[k][b] for k in ('X1', 'X2', 'S1', 'S2', 'S1i', 'S2i', 'Rd1', 'Rd2', 'T1', 'T2', 'Hb', 'V', 'P', 'W3', 'U', 'adjV', 'adjE')}
        tau, alpha = case['prob'][b][P_TAU], case['prob'][b][P_ALPHA]
        # Rd_r; m = 2 nx + 5: V' P_{k+1} V is two nested sums of nx products, then + alpha Hb (2), - P_k, - I, - S_r
        Rd = sr.dual_residuals(g['P'], tau, alpha, g['Hb'], g['V'], g['S1'], g['S2'], nx)
        for r in (1, 2):
            _inside(g[f'Rd{r}'], Rd[r - 1], Rd[r + 1], 2 * nx + 5, f'problem {b} Rd{r}')
            # T_r = -sym(X_r Rd_r S_ri) from the device Rd_r and S_ri; m = 3n (the issue's count; 2n products and the symmetrising sum: 2n + 1 <= 3n)
            T, Tb = sr.predictor_T(g[f'X{r}'], g[f'Rd{r}'], g[f'S{r}i'])
            _inside(g[f'T{r}'], T, Tb, 3 * n, f'problem {b} T{r}')
        # the columns from the device T_r and S_ri; m = 4n (the predictor column: V G V' with G = T1 - T2 is 2n + 1, the two differences and the weight 2n + 3 <= 4n;
        # u_tau: n + 1 for Psi, 3n + 3 in all; u_alpha: 2n + 2 for PhiH, 4n + 4 in all, which the factor 4 absorbs)
        cols, cb = sr.rhs_columns(g['T1'], g['T2'], g['X1'], g['X2'], g['S1i'], g['S2i'], g['Hb'], g['V'], nx)
        _inside(g['W3'][:, :d, :], cols, cb, 4 * n, f'problem {b} W3 [stage, (ab), rhs | u_tau | u_alpha]')
        _inside(g['U'][:, :d, :], cols[:, :, 1:], cb[:, :, 1:], 4 * n, f'problem {b} U [stage, (ab), u_tau | u_alpha]')
        assert not g['W3'][:, d:, :].any() and not g['U'][:, d:, :].any()
        assert np.array_equal(g['U'], g['W3'][:, :, 1:])
        # k_gather alone, from the adjoint pieces the stage kernels left: column j = +-w_ab (adjV[k-1][j] - adjE[k][j])[a, b]; m = 1: one difference (the weight is exact)
        av = np.roll(np.asarray(g['adjV'], sr.LD), 1, axis=0)[:, :, ia, ib]; ae = np.asarray(g['adjE'], sr.LD)[:, :, ia, ib]       # [p, 3, d]
        sign = np.array([1, -1, 1], sr.LD)[None, :, None]
        _inside(g['W3'][:, :d, :], np.moveaxis(sign * wgt * (av - ae), 1, 2), np.moveaxis(wgt * (np.abs(av) + np.abs(ae)), 1, 2), 1, f'problem {b} k_gather')
