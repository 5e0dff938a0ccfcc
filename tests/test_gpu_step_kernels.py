"""Kernel-level check of the second half of an interior-point iteration -- what turns the solved block system into the next iterate: k_stage_rhs in pass 2
(corrector), k_solve_border, k_stage_dir, the inverse Cholesky factors of k_stage_pre, k_eigmin / k_eigmin_lane with the positive-definiteness pre-test, k_ctrl_b,
k_ctrl_c and k_update, and the generic kb_stage_dir / kb_eigmin -- at iterates the SOLVER reached.  A call runs iterations 1 .. K-1 as always and stops inside
iteration K at one of three points (TMPC_DEBUG_FLAG_STOP_ASSEMBLED + tmpc_debug_set_stop_point, include/tunempc_hip_debug.h):
    s1  after pass 1 and k_ctrl_b        s2  pass 2 complete, before k_ctrl_c        s3  iteration K complete
one device call per point, all on one handle with chunk = batch and lanes = 1 (tmpc_debug_get_array reads lane 0).

Every layer is compared with tests/step_reference.py (numpy, np.longdouble) evaluated on that layer's OWN device inputs: |device - reference| <= 4 gamma_m * bound
entrywise, with m derived at each assert (tests/test_gpu_schur_assembly.py explains the form).  Main-phase cases: the shapes and seeds of
tests/schur_assembly_cases.py, the small ones once more with the generic stage kernels.  Centering cases: the first centering iteration and the first chord step
of three shapes, found by a scouting run on the same handle configuration (pass 1 is skipped, pass 2 solves three columns, the pre-test asks two thresholds).

The rows of the G / C multipliers (k_phi_dir, k_phi_steps, k_phi_update) are in tests/test_gpu_phi_kernels.py, those of Step 3 (k_t3_dir, k_t3_steps, k_t3_update) in tests/test_gpu_t3_kernels.py.  Not covered here: the
double-double tight phase (k_dd_aug_fill with it), the bodies as instantiated inside the persistent kernel, and the decisions of k_ctrl_d."""
import numpy as np
import pytest

import schur_reference as sr
import step_reference as st
from schur_assembly_cases import make_problem, solved_members
from step_kernel_cases import (CENTER_CASES, I_CHOLBAD, I_CHORD, I_LOWP, I_NSHIFT, I_PHASE, I_REG, I_SHIFT0, IS, MAIN_CASES, NPART, P_AD, P_ALPHA, P_AP, P_BAA, P_BTA, P_BTT, P_CORR0,
                               P_DALPHA, P_DINF, P_DTAU, P_MU, P_MUT, P_PINF, P_RAWSTEP, P_RD0, P_S0, P_SB00, P_SB01, P_SB11, P_SIGMU, P_STEPN, P_SXS, P_TAU, P_X0, PH_CENTER, PH_DONE,
                               PH_MAIN, PS, Q_DH2, Q_DP2, Q_DXDS, Q_DXS, Q_HBG, Q_M2, Q_P2, Q_TRT2, Q_XDS, TRACE_LEN, TRACE_W, eig_thresholds)
from test_gpu_schur_assembly import _inside

pytestmark = pytest.mark.gpu

LD = sr.LD
FLAG_STOP_ASSEMBLED, FLAG_GENERIC_STAGE = 8, 64
STOP_AFTER_PASS1, STOP_BEFORE_STEP, STOP_AFTER_STEP = 1, 2, 3
# which-codes of tmpc_debug_get_array (include/tunempc_hip_debug.h)
CODES = dict(part=4, W3=7, U=8, X1=9, X2=10, S1=11, S2=12, P=13, V=14, Hb=15, S1i=16, S2i=17, Rd1=18, Rd2=19, T1=20, T2=21, Z=25, prob=26, trace=27, dP=28,
             dX1=29, dX2=30, dS1=31, dS2=32, c1=33, c2=34, L1i=35, L2i=36, LX1i=37, LX2i=38, Wm=39, eigmin=40, TU=41)
# the factor by which the device's Newton residual may exceed that of a dense fp64 LAPACK solve of the same system (test_newton_equations): the largest ratio of
# profiles/step_kernel_residuals.txt (tests/tools/step_kernel_residuals.py) rounded up to the next power of ten -- taken per kind of step, because two kinds are
# inexact Newton steps BY DESIGN and one factor for all would be theirs: 'fp64' a step on a new fp64 factorisation; 'float32' a main-phase iteration whose
# Schur-complement updates and triangular solves ran in float32 (I_LOWP, Opts::lowp_switch); 'chord' a centering step on the factorisation of an earlier iterate
NEWTON_RESIDUAL_FACTOR = dict(fp64=1e2, float32=1e7, chord=1e9)      # largest ratios there: 33.1, 1.27e6, 7.44e8

PARAMS = MAIN_CASES + CENTER_CASES
_STATS = {}          # per case: what the checks that look across the cases need (test_cases_cover_both_answers_and_unequal_steps)


def _id(prm):
    (nb, p, nx, mb), k, generic = prm
    return f'nb{nb}-p{p}-nx{nx}-mb{mb}-' + (f'K{k}' if isinstance(k, int) else k) + ('-generic' if generic else '')


def _snapshot(h, nb, p, nx, n, dp):
    shp = dict(part=(p, NPART), W3=(p, dp, 3), U=(p, dp, 2), TU=(p, dp, 2), Z=(p, dp), P=(p, nx, nx), dP=(p, nx, nx), V=(p, nx, n), prob=(PS,), trace=(TRACE_LEN, TRACE_W),
               Wm=(p, 4, n, n), eigmin=(p, 4))
    c = {}
    for name, code in CODES.items():
        s = (nb,) + shp.get(name, (p, n, n))
        c[name] = h.debug_array(code, 0, int(np.prod(s))).reshape(s)
    c['iprob'] = h.debug_iprob(0, nb * IS).reshape(nb, IS)
    return c


def run_case(prm):
    """the device calls of one case: -> dict(shape, K, n, d, dp, generic, solved, s1, s2, s3[, s2x: pass 2 once more with the pre-test off])"""
    from tunempc_amd._lib import HipConvexifier
    shape, K, generic = prm
    nb, p, nx, mb = shape
    n = nx + mb; d = nx * (nx + 1) // 2; dp = (d + 15) // 16 * 16
    A, B, H = make_problem(shape)
    c = dict(shape=shape, kind=K, n=n, d=d, dp=dp, generic=generic, solved=solved_members(shape), absent=False)
    b0 = c['solved'][0]
    if not isinstance(K, int):
        # scouting run: the whole solve on the launch sequence (what the stop flag forces), then column 1 of the trace: phase + 0.25 * chord
        h = HipConvexifier(p, nx, mb, chunk=nb, lanes=1)
        h.set_tuning(graph=0, persistent=0)
        h.convexify_batch(A, B, H)
        col = h.debug_array(CODES['trace'], 0, nb * TRACE_LEN * TRACE_W).reshape(nb, TRACE_LEN, TRACE_W)[b0, :, 1]
        h.close()
        hit = np.nonzero(col == (1.0 if K == 'center' else 1.25))[0]
        if len(hit) == 0:
            assert K == 'chord', 'the scouting run never reached the centering phase'
            c['absent'] = True           # this run takes no chord step
            return c
        K = int(hit[0]) + 1
    c['K'] = K
    h = HipConvexifier(p, nx, mb, chunk=nb, lanes=1, flags=FLAG_STOP_ASSEMBLED | (FLAG_GENERIC_STAGE if generic else 0))
    assert h.chunk == nb
    for name, point in (('s1', STOP_AFTER_PASS1), ('s2', STOP_BEFORE_STEP), ('s3', STOP_AFTER_STEP)):
        h.debug_set_stop_point(K, point)
        h.convexify_batch(A, B, H)
        c[name] = _snapshot(h, nb, p, nx, n, dp)
    if 8 < n <= 32 and not generic:      # k_eigmin: every eigenvalue, no pre-test
        h.set_tuning(eig_pretest=0)
        h.debug_set_stop_point(K, STOP_BEFORE_STEP)
        h.convexify_batch(A, B, H)
        c['s2x'] = _snapshot(h, nb, p, nx, n, dp)
    h.close()
    return c


@pytest.fixture(scope='module', params=PARAMS, ids=_id)
def case(request):
    c = run_case(request.param)
    _STATS[request.param] = stats(c)
    return c


def members(c):
    """(b, phase, chord) of the members that iterate at the stop"""
    if c['absent']:
        return []
    ip = c['s2']['iprob']
    return [(b, int(ip[b, I_PHASE]), int(ip[b, I_CHORD])) for b in c['solved'] if ip[b, I_PHASE] != PH_DONE]


def eig_kernel_tol(c):
    """tolerance / scale of the kernel that computes the step-length eigenvalues of this case, the one tests/test_gpu_parity.py holds its primitive to:
    1e-12 for k_eigmin (tridiag_min_eig), 1e-13 for k_eigmin_lane (n <= 8) and kb_eigmin (big_eig_extremes)"""
    return 1e-12 if (8 < c['n'] <= 32 and not c['generic']) else 1e-13


def eig_answers(c, snap, b, phase, pass2):
    """per entry of eigmin [p, 4]: (device, ref = eigvalsh(device Wm)[0], scale, kind), kind 'exact' (within the tolerance of ref) or 'bound' (exactly -1 / theta
    of a threshold of the phase, with ref > -1 / theta); asserts that every entry is one of the two and that pass 1 / the other kernels never report a bound"""
    ev = np.linalg.eigvalsh(snap['Wm'][b])
    ref, scale = ev[..., 0], np.abs(ev).max(-1)
    got = snap['eigmin'][b]
    tol = eig_kernel_tol(c)
    pretest = pass2 and tol == 1e-12
    th = eig_thresholds(phase)
    kinds = np.empty(got.shape, object)
    for idx in np.ndindex(got.shape):
        g, r, s = got[idx], ref[idx], scale[idx]
        hit = [t for t in th if g == -1.0 / t] if pretest else []
        if hit:
            assert r > -1.0 / hit[0], (idx, g, r, 'the sweep answered "positive definite" wrongly')
            kinds[idx] = 'bound'
        else:
            assert abs(g - r) <= tol * max(s, 1e-300), (idx, g, r, s)
            kinds[idx] = 'exact'
        if pretest and r > -1.0 / th[0] * (1.0 - 1e-9):
            assert g == -1.0 / th[0], (idx, g, r, 'safely inside the longest threshold, yet not answered by the sweep')
    return got, ref, scale, kinds


def stats(c):
    out = dict(kinds=set(), unequal=False, chord=False)
    for b, phase, chord in members(c):
        if 8 < c['n'] <= 32 and not c['generic']:
            out['kinds'] |= set(eig_answers(c, c['s2'], b, phase, True)[3].ravel())
        pr = c['s3']['prob'][b]
        out['unequal'] |= bool(pr[P_AP] != pr[P_AD])
        out['chord'] |= bool(chord)
    return out


def _g(snap, b):
    return {k: v[b] for k, v in snap.items()}


# ------------------------------------------------------------------------------------------------------------------------------ 1. state at the stop
def test_state_at_the_stop_points(case):
    """phase, no lift, no frozen pivot; row K of the trace absent at s1 and s2, present at s3; and what iteration K does not write between two points is
    bit-identical across the calls: the whole iterate, the stage data and every scalar but (dtau, dalpha) between s1 and s2; the direction, the step-length
    matrices and their eigenvalues between s2 and s3 -- the run-to-run reproducibility of the solver"""
    if case['absent']:
        return
    K, kind = case['K'], case['kind']
    b0 = case['solved'][0]
    assert len(members(case)) >= 1
    for b, phase, chord in members(case):
        for s in ('s1', 's2'):
            ip = case[s]['iprob'][b]
            assert ip[I_PHASE] == phase and ip[I_CHORD] == chord and ip[I_REG] == 0 and ip[I_NSHIFT] == ip[I_SHIFT0], (s, ip)
            tr = case[s]['trace'][b]
            assert tr[K - 2, 0] == K - 1 if K > 1 else True
            assert not tr[K - 1:].any(), (s, tr[K - 1])
        row = case['s3']['trace'][b][K - 1]
        assert row[0] == K and row[1] == phase + 0.25 * chord and not case['s3']['trace'][b][K:].any(), row
        if b == b0:
            want = dict(center=(PH_CENTER, 0), chord=(PH_CENTER, 1)).get(kind, (PH_MAIN, 0))
            assert (phase, chord) == want, (phase, chord, want)
        a, z = _g(case['s1'], b), _g(case['s2'], b)
        for k in ('X1', 'X2', 'S1', 'S2', 'P', 'V', 'Hb', 'S1i', 'S2i', 'Rd1', 'Rd2', 'L1i', 'L2i', 'LX1i', 'LX2i'):
            assert np.array_equal(a[k], z[k]), (k, 's1 vs s2')
        keep = np.ones(PS, bool); keep[[P_DTAU, P_DALPHA]] = False
        if phase != PH_MAIN and not chord:
            keep[[P_SB00, P_SB01, P_SB11]] = False          # a centering iteration with a new factorisation forms the border matrix in pass 2
        assert np.array_equal(a['prob'][keep], z['prob'][keep]), np.nonzero(a['prob'] != z['prob'])
        if phase == PH_MAIN or chord:
            assert np.array_equal(a['TU'], z['TU']) and np.array_equal(a['U'], z['U'])       # pass 2 of the main phase and a chord step re-use U and T^-1 U
        y = _g(case['s3'], b)
        for k in ('dX1', 'dX2', 'dS1', 'dS2', 'dP', 'Wm', 'eigmin', 'T1', 'T2', 'c1', 'c2', 'TU', 'Z', 'S1i', 'S2i', 'Rd1', 'Rd2'):
            assert np.array_equal(z[k], y[k]), (k, 's2 vs s3')


# ------------------------------------------------------------------------------------------------------------------------------ 2. inverse factors
def test_inverse_cholesky_factors(case):
    """L_r^-1 and LX_r^-1 of k_stage_pre / kb_stage_pre: lower triangular, and ||L^-1 S L^-T - I||_max <= 4 gamma_{3n} cond_2(S) (likewise X); m = 3n: n terms in each
    of the factorisation, the triangular inverse and the product -- the form of test_gpu_schur_assembly.py::test_inverses"""
    n = case['n']
    I = np.eye(n, dtype=LD)
    for b, phase, chord in members(case):
        g = _g(case['s2'], b)
        for name, mat in (('L1i', 'S1'), ('L2i', 'S2'), ('LX1i', 'X1'), ('LX2i', 'X2')):
            Li, S = g[name], g[mat]
            assert not np.triu(Li, 1).any(), name
            assert np.all(np.diagonal(Li, axis1=1, axis2=2) > 0), name
            LiL = np.asarray(Li, LD)
            res = np.abs(LiL @ np.asarray(S, LD) @ np.swapaxes(LiL, 1, 2) - I).max(axis=(1, 2))
            lim = 4 * sr.gamma(3 * n) * np.linalg.cond(S)
            assert np.all(res <= lim), (b, name, res, lim)


# ------------------------------------------------------------------------------------------------------------------------------ 3. pass-2 right-hand side
def test_pass2_T_and_partial_sums(case):
    """T_r of pass 2 from device X, S^-1, Rd, c_r and P_SIGMU -- the corrector exactly in the main phase (while centering c_r still holds the term of the last
    main-phase iteration: a kernel that subtracted it would be found); m = 3n + 2: the 3n of the predictor (test_right_hand_sides), sigma mu S^-1 and c_r.
    Q_TRT2 = tr T2 (m = n), Q_HBG = <Hb, T1 - T2> (m = n^2 + 1) from the device T_r."""
    n = case['n']
    for b, phase, chord in members(case):
        g = _g(case['s2'], b)
        sigmu = g['prob'][P_SIGMU]
        assert sigmu > 0.0
        if phase != PH_MAIN:
            assert sigmu == g['prob'][P_MUT] and (g['c1'].any() or case['K'] == 1)
        for r in (1, 2):
            T, Tb = st.corrector_T(g[f'X{r}'], g[f'Rd{r}'], g[f'S{r}i'], sigmu, g[f'c{r}'] if phase == PH_MAIN else None)
            _inside(g[f'T{r}'], T, Tb, 3 * n + 2, f'problem {b} pass-2 T{r}')
        q, qb = st.rhs_partials(g['T1'], g['T2'], g['Hb'])
        _inside(g['part'][:, Q_TRT2], q[:, 0], qb[:, 0], n, f'problem {b} Q_TRT2')
        _inside(g['part'][:, Q_HBG], q[:, 1], qb[:, 1], n * n + 1, f'problem {b} Q_HBG')


# ------------------------------------------------------------------------------------------------------------------------------ 4. border solve
def _border(case, g, b, pass1, three, what):
    """k_solve_border of one pass from the device's solved columns"""
    p, nx, d, dp = case['shape'][1], case['shape'][2], case['d'], case['dp']
    pr = g['prob']
    mdot = p * dp + 1                                              # a border sum runs over the padded vectors of all stages, one fma per entry
    if three:
        assert np.array_equal(g['TU'], g['W3'][:, :, 1:]) and np.array_equal(g['Z'], g['W3'][:, :, 0]), what + ': TU / Z are bit copies of the solved W3 columns'
        SB, SBb = st.border_matrix(pr[P_BTT], pr[P_BTA], pr[P_BAA], g['U'], g['TU'])
        _inside(pr[[P_SB00, P_SB01, P_SB11]], SB, SBb, mdot, what + ' SB00 / SB01 / SB11')
    sig, corr0 = (0.0, 0.0) if pass1 else (pr[P_SIGMU], pr[P_CORR0])
    rb, rbb = st.border_rhs(g['part'][:, Q_TRT2], g['part'][:, Q_HBG], g['Z'], g['U'], sig, corr0, pr[P_S0], pr[P_X0], pr[P_RD0])
    db, dbb = st.border_solution(pr[[P_SB00, P_SB01, P_SB11]], rb, rbb)
    # m: the sums of rb (p dp + p + 6 with t0), then 3 operations of the numerator, 3 of the determinant and the division
    _inside(pr[[P_DTAU, P_DALPHA]], db, dbb, mdot + p + 13, what + ' dtau / dalpha')
    dP, dPb = st.direction_P(g['Z'], g['TU'], pr[P_DTAU], pr[P_DALPHA], nx)
    _inside(g['dP'], dP, dPb, 4, what + ' dP')                    # m = 4: two products, two differences
    assert np.array_equal(g['dP'], np.swapaxes(g['dP'], 1, 2)), what + ': dP is exactly symmetric'


def test_border_solve(case):
    """P_SB*, (dtau, dalpha) and dP of both passes from the device's solved W3 / Z, U, partial sums and scalars; TU and Z bit copies of the W3 columns; dP exactly
    symmetric, packed over the row-major upper triangle (direction_P unpacks with np.triu_indices).  Main phase: pass 1 solves three columns, pass 2 one.
    Centering: pass 2 solves all three, a chord step only the right-hand side (TU and SB* stay: test_state_at_the_stop_points)."""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _border(case, _g(case['s1'], b), b, True, True, f'problem {b} pass 1')
            _border(case, _g(case['s2'], b), b, False, False, f'problem {b} pass 2')
        else:
            _border(case, _g(case['s2'], b), b, False, not chord, f'problem {b} centering pass 2')
            if chord:
                a, z = _g(case['s1'], b), _g(case['s2'], b)
                assert np.array_equal(a['prob'][[P_SB00, P_SB01, P_SB11]], z['prob'][[P_SB00, P_SB01, P_SB11]])


# ------------------------------------------------------------------------------------------------------------------------------ 5. directions
def _directions(case, g, b, pass1, what):
    nx, n = case['shape'][2], case['n']
    pr = g['prob']
    dM, dMb = st.direction_M(g['dP'], pr[P_DALPHA], g['Hb'], g['V'], nx)
    Ldy, Ldyb = st.linear_parts(dM, dMb, pr[P_DTAU])
    X, S, dX, dS = (g['X1'], g['X2']), (g['S1'], g['S2']), (g['dX1'], g['dX2']), (g['dS1'], g['dS2'])
    for r in (0, 1):
        # dS_r; m = 2 nx + 5: dM is two nested sums of nx products, + dalpha Hb (2), - dP_k (1); then dtau I - dM and + Rd
        v, vb = st.direction_S(Ldy[r], Ldyb[r], g[f'Rd{r + 1}'])
        _inside(dS[r], v, vb, 2 * nx + 5, what + f' dS{r + 1}')
        # dX_r from the device T_r; m = (2 nx + 4) + (2n + 1) + 2: the roundings of Ldy ride through the product X Ldy S^-1 (2n terms and the half-sum), then T - X - .
        v, vb = st.direction_X(g[f'T{r + 1}'], X[r], Ldy[r], Ldyb[r], g[f'S{r + 1}i'])
        _inside(dX[r], v, vb, 2 * nx + 2 * n + 7, what + f' dX{r + 1}')
        # step-length matrices from the device dS, dX and inverse factors; m = 2n + 1: two nested sums of n products and the half-sum.  Slot 2r dual, 2r + 1 primal
        v, vb = st.step_matrix(g[f'L{r + 1}i'], dS[r])
        _inside(g['Wm'][:, 2 * r], v, vb, 2 * n + 1, what + f' Wm slot {2 * r} (dual)')
        v, vb = st.step_matrix(g[f'LX{r + 1}i'], dX[r])
        _inside(g['Wm'][:, 2 * r + 1], v, vb, 2 * n + 1, what + f' Wm slot {2 * r + 1} (primal)')
        if pass1:
            v, vb = st.corrector_term(dX[r], dS[r], g[f'S{r + 1}i'])
            _inside(g[f'c{r + 1}'], v, vb, 2 * n + 1, what + f' c{r + 1}')
            assert np.array_equal(g[f'c{r + 1}'], np.swapaxes(g[f'c{r + 1}'], 1, 2))
    assert np.array_equal(g['Wm'], np.swapaxes(g['Wm'], 2, 3)), what + ': Wm is exactly symmetric'
    # the seven partial sums from the device direction; m: a sum over both cones 2 n^2 + 1; over P nx^2; DH2: dh = dM - (dalpha / alpha) M carries 2 nx + 8
    # roundings, squared twice that and one, then n^2 terms; M2: M = S1 + Rd1 + I (2), squared, n^2 terms
    v, vb = st.partial_sums(dX, dS, X, S, g['dP'], g['P'], dM, dMb, g['S1'], g['Rd1'], pr[P_DALPHA], pr[P_ALPHA])
    ms = (2 * n * n + 1,) * 3 + (nx * nx,) * 2 + (n * n + 4 * nx + 17, n * n + 5)
    for j, (q, m) in enumerate(zip((Q_DXS, Q_XDS, Q_DXDS, Q_DP2, Q_P2, Q_DH2, Q_M2), ms)):
        _inside(g['part'][:, q], v[:, j], vb[:, j], m, what + f' partial sum {st.PART_NAMES[j]}')


def test_directions(case):
    """dS_r, dX_r, the four step-length matrices, the corrector term (pass 1) and the seven partial sums of k_stage_dir / kb_stage_dir, both passes, from the device
    dP, dtau, dalpha, V, Hb, X, S^-1, Rd, T, L^-1, LX^-1"""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _directions(case, _g(case['s1'], b), b, True, f'problem {b} pass 1')
        _directions(case, _g(case['s2'], b), b, False, f'problem {b} pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 6. Newton equations
def newton_residuals(case, b, phase):
    """relative residual of the three linear primal equations (r_tau, r_alpha, r_P of k_ctrl_a) at X + dX, x0 + dx0 with (device pass-2 direction, the direction of a
    dense fp64 LAPACK solve from the same device iterate: step_reference.newton_iteration); the reference floored at 2^-53, one rounding of the residual's own sums"""
    g = _g(case['s2'], b)
    nx = case['shape'][2]
    pr = g['prob']
    ds0 = LD(pr[P_DALPHA]) + LD(pr[P_RD0])
    dx0 = LD(pr[P_SIGMU]) / LD(pr[P_S0]) - LD(pr[P_X0]) - LD(pr[P_X0]) * ds0 / LD(pr[P_S0]) - LD(pr[P_CORR0])

    def rel(dX1, dX2, dx0_):
        rt, ra, rP, scale = st.primal_residuals(np.asarray(g['X1'], LD) + np.asarray(dX1, LD), np.asarray(g['X2'], LD) + np.asarray(dX2, LD), LD(pr[P_X0]) + LD(dx0_),
                                                g['Hb'], g['V'], nx)
        return float(max(abs(rt), abs(ra), np.abs(rP).max()) / scale)
    it = dict(X1=g['X1'], X2=g['X2'], S1=g['S1'], S2=g['S2'], P=g['P'], V=g['V'], Hb=g['Hb'], tau=pr[P_TAU], alpha=pr[P_ALPHA], x0=pr[P_X0], s0=pr[P_S0],
              mu_t=pr[P_MUT], phase=phase)
    _, info = st.newton_iteration(it)
    return rel(g['dX1'], g['dX2'], dx0), max(rel(info['dX'][0], info['dX'][1], info['dx0']), 2.0 ** -53)


def step_kind(case, b, chord):
    return 'chord' if chord else ('float32' if case['s2']['iprob'][b, I_LOWP] else 'fp64')


def test_newton_equations(case):
    """The pass-2 direction solves the linearised primal equations: r_tau, r_alpha and r_P, linear in the iterate, vanish at X + dX, x0 + dx0 up to the error of the
    solve -- the one check that ties pass-2 gather, block solve, border, scatter and dM together.  That error has no rounding bound (it depends on the conditioning
    of the Schur matrix), so it is measured against a dense fp64 LAPACK solve from the same device iterate: the device's relative residual may exceed the
    reference's by NEWTON_RESIDUAL_FACTOR of its kind of step (the block factorisation multiplies by inverted diagonal tiles, tmpc_schur.h: ~sqrt(cond D_k) eps
    against a substitution; a float32 factorisation and a chord step solve the equations only as well as their factor fits the iterate).  A case whose reference residual is itself above 1e-6 is ill-posed for this check."""
    for b, phase, chord in members(case):
        dev, ref = newton_residuals(case, b, phase)
        kind = step_kind(case, b, chord)
        print(f'newton-residual {_id((case["shape"], case["kind"], case["generic"]))} problem {b} {kind}: device {dev:.3e} reference {ref:.3e} ratio {dev / ref:.3g}')
        assert ref <= 1e-6, (b, ref)
        assert dev <= NEWTON_RESIDUAL_FACTOR[kind] * ref, (b, kind, dev, ref, dev / ref)


# ------------------------------------------------------------------------------------------------------------------------------ 7. step-length eigenvalues
def test_step_length_eigenvalues(case):
    """eigmin against eigvalsh of the device's own Wm at the tolerance tests/test_gpu_parity.py holds each primitive to.  Pass 1 and the kernels without a pre-test
    (k_eigmin_lane, kb_eigmin) report every eigenvalue; so does k_eigmin with eig_pretest = 0.  With the default a pass-2 entry of k_eigmin is the eigenvalue or
    exactly -1 / theta of a threshold of its phase, then with ref > -1 / theta (the sweep's answer was true), and an entry safely inside the longest threshold must be
    a bound (the pre-test runs): eig_answers."""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            kinds = eig_answers(case, case['s1'], b, phase, False)[3]
            assert np.all(kinds == 'exact')
        eig_answers(case, case['s2'], b, phase, True)
        if 's2x' in case:
            x = case['s2x']
            assert np.array_equal(x['Wm'][b], case['s2']['Wm'][b])            # the pre-test changes no iterate: same matrices bit for bit
            ev = np.linalg.eigvalsh(x['Wm'][b])
            assert np.all(np.abs(x['eigmin'][b] - ev[..., 0]) <= 1e-12 * np.maximum(np.abs(ev).max(-1), 1e-300))


# ------------------------------------------------------------------------------------------------------------------------------ 8. control kernels
def _close(got, ref, bound, m, what):
    _inside(np.array([got], float), np.array([ref], LD), np.array([bound], LD), m, what)


def test_control_kernels(case):
    """k_ctrl_b (s1: sigma mu and P_CORR0) and k_ctrl_c (s3: step lengths, scalar updates, trace row) recomputed from the device eigmin, partial sums and scalars;
    each a handful of operations, m counted at the assert.  From the EXACT eigenvalues of Wm in the place of the device's eigmin the step lengths are the same: exactly
    1.0 where the device clipped (the pre-test's claim that a bound leads to the same clipped step), and within the eigenvalue's own tolerance elsewhere.  ap comes from
    the primal minima (slots 1, 3), ad from the dual ones (slots 0, 2): step_reference.eig_minima."""
    p, n = case['shape'][1], case['n']
    N = 2 * p * n + 1
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            g = _g(case['s1'], b); pr = g['prob']
            r = st.sigma_rule(g['eigmin'], g['part'][:, Q_DXS], g['part'][:, Q_XDS], g['part'][:, Q_DXDS], pr[P_SXS], pr[P_X0], pr[P_S0], pr[P_MU], pr[P_MUT],
                              pr[P_DALPHA], pr[P_RD0], N)
            # m: three sums over p stages, ds0 (1), dx0 (3), two divisions for the steps, mu_aff (12), the ratio, its square and the product with mu: 3p + 24
            _close(pr[P_SIGMU], r['sigmu'], r['sigmu_b'], 3 * p + 24, f'problem {b} P_SIGMU')
            _close(pr[P_CORR0], r['corr0'], r['corr0_b'], 6, f'problem {b} P_CORR0')             # ds0 (1), dx0 (3), product and division
        g = _g(case['s2'], b); pr = g['prob']; y = case['s3']['prob'][b]
        r = st.step_rule(phase, g['eigmin'], g['part'][:, Q_DH2], g['part'][:, Q_M2], pr[P_SIGMU], pr[P_CORR0], pr[P_X0], pr[P_S0], pr[P_TAU], pr[P_ALPHA],
                         pr[P_DTAU], pr[P_DALPHA], pr[P_RD0])
        # raw step: one division (of x0 / dx0: dx0 carries 6 roundings); damped: gamma (2) and the product
        _close(y[P_RAWSTEP], r['rawstep'], abs(r['rawstep']), 8, f'problem {b} P_RAWSTEP')
        _close(y[P_AP], r['ap'], abs(r['ap']), 12, f'problem {b} P_AP')
        _close(y[P_AD], r['ad'], abs(r['ad']), 12, f'problem {b} P_AD')
        _close(y[P_STEPN], r['stepn'], abs(r['stepn']), 2 * p + 2, f'problem {b} P_STEPN')           # two sums over p stages, division, square root
        # the scalar updates with the device's own step lengths; m = 8: dx0 (6), product, sum
        ap, ad = LD(y[P_AP]), LD(y[P_AD])
        _close(y[P_X0], LD(pr[P_X0]) + ap * r['dx0'], LD(pr[P_X0]) + ap * r['dx0_b'], 8, f'problem {b} x0')
        _close(y[P_S0], LD(pr[P_S0]) + ad * r['ds0'], LD(pr[P_S0]) + ad * r['ds0_b'], 4, f'problem {b} s0')
        _close(y[P_TAU], LD(pr[P_TAU]) + ad * LD(pr[P_DTAU]), abs(LD(pr[P_TAU])) + abs(ad * LD(pr[P_DTAU])), 2, f'problem {b} tau')
        _close(y[P_ALPHA], LD(pr[P_ALPHA]) + ad * LD(pr[P_DALPHA]), abs(LD(pr[P_ALPHA])) + abs(ad * LD(pr[P_DALPHA])), 2, f'problem {b} alpha')
        row = case['s3']['trace'][b][case['K'] - 1]
        want = [case['K'], phase + 0.25 * chord, pr[P_MU], pr[P_TAU], pr[P_PINF], pr[P_DINF], y[P_AP], y[P_RAWSTEP] if phase == PH_CENTER else y[P_AD], y[P_STEPN],
                float(case['s3']['iprob'][b, I_NSHIFT] + case['s3']['iprob'][b, I_CHOLBAD])]
        assert np.array_equal(row, np.array(want)), (row, want)         # copies: bit for bit (tau, mu, pinf, dinf: of the iterate the step started from)
        # ... and from the exact eigenvalues
        ev = np.linalg.eigvalsh(g['Wm'])
        ex, scale = ev[..., 0], np.abs(ev).max(-1)
        rx = st.step_rule(phase, ex, g['part'][:, Q_DH2], g['part'][:, Q_M2], pr[P_SIGMU], pr[P_CORR0], pr[P_X0], pr[P_S0], pr[P_TAU], pr[P_ALPHA], pr[P_DTAU],
                          pr[P_DALPHA], pr[P_RD0])
        tol = eig_kernel_tol(case)
        for name, idx, cols in (('ap', P_AP, (1, 3)), ('ad', P_AD, (0, 2))):
            if y[idx] == 1.0:
                assert rx[name] == 1.0, (name, rx[name])
            else:
                # a = -damp / lambda: d a / a = d lambda / |lambda|, with |d lambda| <= tol * scale of the matrix that holds the minimum (gamma depends on it once more)
                k = np.unravel_index(np.argmin(ex[:, list(cols)]), ex[:, list(cols)].shape)
                lam, sc = ex[:, list(cols)][k], scale[:, list(cols)][k]
                assert abs(float(rx[name]) - y[idx]) <= 4 * tol * sc / abs(lam) * y[idx] + 1e-15, (name, float(rx[name]), y[idx])


# ------------------------------------------------------------------------------------------------------------------------------ 9. update
def test_update(case):
    """X_r, S_r, P at s3 from the iterate and direction of s2 with the step lengths of s3: X moves by ap, S and P by ad; m = 3 (product, sum, half-sum); the results
    exactly symmetric; a member that left at the pre-check (PH_DONE) untouched bit for bit"""
    if case['absent']:
        return
    for b, phase, chord in members(case):
        g, y = _g(case['s2'], b), _g(case['s3'], b)
        ap, ad = y['prob'][P_AP], y['prob'][P_AD]
        assert ap > 0.0 and ad > 0.0
        for name, dname, a, sym in (('X1', 'dX1', ap, True), ('X2', 'dX2', ap, True), ('S1', 'dS1', ad, True), ('S2', 'dS2', ad, True), ('P', 'dP', ad, False)):
            v, vb = st.update(g[name], g[dname], a, symmetric=sym)
            _inside(y[name], v, vb, 3, f'problem {b} updated {name}')
            assert np.array_equal(y[name], np.swapaxes(y[name], 1, 2)), name
            assert not np.array_equal(y[name], g[name]), name + ' did not move'
    idle = [b for b in range(case['shape'][0]) if b not in [m[0] for m in members(case)]]
    for b in idle:
        assert case['s3']['iprob'][b, I_PHASE] == PH_DONE
        for name in ('X1', 'X2', 'S1', 'S2', 'P'):
            assert np.array_equal(case['s2'][name][b], case['s3'][name][b]), (b, name)
            assert np.array_equal(case['s1'][name][b], case['s3'][name][b]), (b, name)
    if case['shape'] == (3, 3, 5, 2) and isinstance(case['kind'], int):
        assert idle == [1]


# ------------------------------------------------------------------------------------------------------------------------------ across the cases
def test_cases_cover_both_answers_and_unequal_steps():
    """across the cases: k_eigmin's pass 2 gives both kinds of answer (eigenvalue, bound); some step has ap != ad (test_update would not tell ap from ad otherwise);
    some run takes a chord step"""
    for prm in PARAMS:
        if prm not in _STATS:
            _STATS[prm] = stats(run_case(prm))
    kinds = set().union(*(s['kinds'] for s in _STATS.values()))
    assert kinds == {'exact', 'bound'}, kinds
    assert any(s['unequal'] for s in _STATS.values())
    assert any(s['chord'] for s in _STATS.values())
