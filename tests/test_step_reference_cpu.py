"""tests/step_reference.py against the CPU oracle, against its own rounding bounds, and against mutated copies of itself (no device).

The GPU test (tests/test_gpu_step_kernels.py) compares every kernel of the second half of an interior-point iteration with this reference inside 4 gamma_m * bound.
Here: newton_iteration, built from the layer functions, walks the oracle's path; the same formulas in plain fp64 numpy (BLAS: another summation order) stay inside
those bounds with the GPU test's own operation counts, so a correct kernel can; and each numerical mutation of profiles/step_kernel_mutations.txt, applied to the
reference, leaves them on the same inputs, so a wrong kernel cannot."""
import numpy as np
import pytest

import convexify_oracle as co
import schur_reference as sr
import step_reference as st
from schur_assembly_cases import SMALL_CASES, make_problem, solved_members
from step_kernel_cases import CENTER_SHAPES, LARGE_CASES, MAIN_CASES, PH_CENTER, PH_MAIN, eig_thresholds
from test_schur_reference_cpu import _chol_inverse_fp64, _rel, _spd

LD = np.longdouble
f64 = np.float64


def _start(A, B, Hs):
    """the oracle's initial point (convexify_oracle.sdp_step1)"""
    p, nx, _ = A.shape
    n = Hs.shape[1]
    s, sbeta = co.auto_scaling(Hs)
    Hb = s * Hs
    I = np.eye(n)
    tau, alpha = 2.0, 1.0 / sbeta
    X = np.broadcast_to(I / (p * n), (p, n, n))
    return dict(X1=X.copy(), X2=X.copy(), S1=np.broadcast_to(I, (p, n, n)).copy(), S2=tau * I - alpha * Hb, P=np.zeros((p, nx, nx)), V=np.concatenate([A, B], axis=2),
                Hb=Hb, tau=tau, alpha=alpha, x0=1.0 / (p * n), s0=alpha, mu_t=None, phase=0, tol=co.DEFAULT_OPTS['tol'])


def _walk(shape, iters):
    A, B, H = make_problem(shape)
    b = solved_members(shape)[0]
    it = _start(A[b], B[b], co.symmetrize(H[b]))
    out = []
    for _ in range(iters):
        nxt, info = st.newton_iteration(it)
        out.append((it, info))
        it = nxt
    return A[b], B[b], co.symmetrize(H[b]), out


@pytest.mark.parametrize('shape', SMALL_CASES)
def test_newton_iteration_walks_the_oracles_path(shape):
    """newton_iteration, started from the oracle's initial point, reproduces mu and tau of sdp_step1(..., trace=) for the first seven iterations -- with the measure and
    the tolerance of tests/test_schur_reference_cpu.py's tie to the oracle: _rel (largest error over largest value) <= 1e-13.  (Two fp64 solvers of one path part
    ways at the rate the Schur matrix loses condition: relative to mu ITSELF, which falls by two to five orders in these iterations, the seventh value differs by up to 1e-8.)"""
    A, B, Hs, steps = _walk(shape, 7)
    trace = []
    co.sdp_step1(A, B, Hs, dict(max_iter=8), trace=trace)
    assert all(t['phase'] == 0 for t in trace[:7])
    for key, mine in (('mu', [info['mu'] for _, info in steps]), ('tau', [it['tau'] for it, _ in steps])):
        ref = np.array([t[key] for t in trace[:7]])
        assert _rel(np.array(mine), ref) <= 1e-13, (key, _rel(np.array(mine), ref))
    assert steps[6][1]['mu'] < 0.1 * steps[0][1]['mu']            # the path was followed, not stood on


def _layer_inputs(seed, p, nx, mb, condS, condX):
    """synthetic inputs of every layer: SPD X_r, S_r with the given condition numbers, fp64 inverses and inverse factors, random right-hand sides and scalars"""
    rng = np.random.default_rng(seed)
    n = nx + mb; d = nx * (nx + 1) // 2; dp = (d + 15) // 16 * 16
    g = dict(p=p, nx=nx, n=n, d=d, dp=dp)
    g['X1'], g['X2'], g['S1'], g['S2'] = _spd(rng, p, n, condX), _spd(rng, p, n, 3 * condX), _spd(rng, p, n, condS), _spd(rng, p, n, 3 * condS)
    g['V'] = rng.standard_normal((p, nx, n)) / np.sqrt(nx)
    g['Hb'] = co.symmetrize(rng.standard_normal((p, n, n))); g['P'] = co.symmetrize(rng.standard_normal((p, nx, nx)))
    g['tau'], g['alpha'], g['x0'], g['s0'], g['sigmu'], g['corr0'], g['mu'] = 1.7, 0.3, 0.04, 0.3 - 1e-3, 3e-3, 2e-3, 0.05
    g['rd0'] = (g['alpha'] - st.ALPHA_MIN) - g['s0']
    for r in (1, 2):
        S, X = g[f'S{r}'], g[f'X{r}']
        g[f'S{r}i'] = _chol_inverse_fp64(S)
        g[f'L{r}i'] = np.stack([np.linalg.inv(np.linalg.cholesky(S[k])) for k in range(p)])
        g[f'LX{r}i'] = np.stack([np.linalg.inv(np.linalg.cholesky(X[k])) for k in range(p)])
        g[f'c{r}'] = 1e-2 * co.symmetrize(rng.standard_normal((p, n, n)))
    Rd = sr.dual_residuals(g['P'], g['tau'], g['alpha'], g['Hb'], g['V'], g['S1'], g['S2'], nx, f64)
    g['Rd1'], g['Rd2'] = Rd[0], Rd[1]
    pad = np.zeros((p, dp, 1)); pad[:, :d] = 1.0
    g['U'] = rng.standard_normal((p, dp, 2)) * pad; g['TU'] = rng.standard_normal((p, dp, 2)) * pad; g['Z'] = rng.standard_normal((p, dp)) * pad[:, :, 0]
    g['btt'], g['bta'], g['baa'] = (float(np.sum(g['U'][..., 0] * g['TU'][..., 0])) + 2.0, 0.3, float(np.sum(g['U'][..., 1] * g['TU'][..., 1])) + 3.0)
    g['dtau'], g['dalpha'] = 0.21, -0.13
    return g


def _layers(g, dtype, mut=None):
    """every layer of the reference from the inputs g in `dtype`, each layer from the fp64 values of the layer before: {name: (value, bound, m)}; m as derived at
    the asserts of tests/test_gpu_step_kernels.py.  mut: one mutation of profiles/step_kernel_mutations.txt applied to the reference."""
    p, nx, n, dp = g['p'], g['nx'], g['n'], g['dp']
    out = {}
    T = []
    for r in (1, 2):
        c = g[f'c{r}'] if mut != 'rhs_plus_corrector' else -g[f'c{r}']
        v, b = st.corrector_T(g[f'X{r}'], g[f'Rd{r}'], g[f'S{r}i'], g['sigmu'], c, dtype)
        out[f'T{r}'] = (v, b, 3 * n + 2)
        T.append(st.corrector_T(g[f'X{r}'], g[f'Rd{r}'], g[f'S{r}i'], g['sigmu'], g[f'c{r}'], f64)[0])
    v, b = st.rhs_partials(T[0], T[1], g['Hb'], dtype)
    out['trt2'] = (v[:, 0], b[:, 0], n); out['hbg'] = (v[:, 1], b[:, 1], n * n + 1)
    q64 = st.rhs_partials(T[0], T[1], g['Hb'], f64)[0]
    v, b = st.border_matrix(g['btt'], g['bta'], g['baa'], g['U'], g['TU'], dtype)
    out['SB'] = (v, b, p * dp + 1)
    SB64 = st.border_matrix(g['btt'], g['bta'], g['baa'], g['U'], g['TU'], f64)[0]
    rb, rbb = st.border_rhs(q64[:, 0], q64[:, 1], g['Z'], g['U'], g['sigmu'], g['corr0'], g['s0'], g['x0'], g['rd0'], dtype)
    v, b = st.border_solution(SB64, rb, rbb, dtype)
    if mut == 'border_bb_sign_dalpha':
        a_, bb_, c_ = (dtype(x) for x in SB64)
        v = np.array([v[0], (a_ * rb[1] + bb_ * rb[0]) / (a_ * c_ - bb_ * bb_)], dtype)
    out['db'] = (v, b, p * dp + p + 14)
    v, b = st.direction_P(g['Z'], g['TU'], g['dtau'], g['dalpha'], nx, dtype)
    out['dP'] = (v, b, 4)
    dP64 = st.direction_P(g['Z'], g['TU'], g['dtau'], g['dalpha'], nx, f64)[0]
    dM, dMb = st.direction_M(dP64, g['dalpha'], g['Hb'], g['V'], nx, dtype)
    Ldy, Ldyb = st.linear_parts(dM, dMb, g['dtau'], dtype)
    dM64, dMb64 = st.direction_M(dP64, g['dalpha'], g['Hb'], g['V'], nx, f64)
    Ldy64, Ldyb64 = st.linear_parts(dM64, dMb64, g['dtau'], f64)
    dS64, dX64 = [], []
    for r in (0, 1):
        v, b = st.direction_S(Ldy[r], Ldyb[r], g[f'Rd{r + 1}'], dtype)
        out[f'dS{r + 1}'] = (v, b, 2 * nx + 5)
        v, b = st.direction_X(T[r], g[f'X{r + 1}'], Ldy[r], Ldyb[r], g[f'S{r + 1}i'], dtype, half_sum=mut != 'dir_dx_no_half_sum',
                              sign=-1 if (mut == 'dir_ldy_sign_r1' and r == 1) else 1)
        out[f'dX{r + 1}'] = (v, b, 2 * nx + 2 * n + 7)
        dS64.append(st.direction_S(Ldy64[r], Ldyb64[r], g[f'Rd{r + 1}'], f64)[0])
        dX64.append(st.direction_X(T[r], g[f'X{r + 1}'], Ldy64[r], Ldyb64[r], g[f'S{r + 1}i'], f64)[0])
    for r in (0, 1):
        Li, LXi = g[f'L{r + 1}i'], g[f'LX{r + 1}i']
        if mut == 'dir_swap_L_LX':
            Li, LXi = LXi, Li
        v, b = st.step_matrix(Li, dS64[r], dtype)
        out[f'W{2 * r}'] = (v, b, 2 * n + 1)
        v, b = st.step_matrix(LXi, dX64[r], dtype)
        out[f'W{2 * r + 1}'] = (v, b, 2 * n + 1)
        v, b = st.corrector_term(dX64[r], dS64[r], g[f'S{2 - r}i' if mut == 'dir_corr_other_cone_Si' else f'S{r + 1}i'], dtype)
        out[f'c{r + 1}'] = (v, b, 2 * n + 1)
    v, b = st.partial_sums(dX64, dS64, (g['X1'], g['X2']), (g['S1'], g['S2']), dP64, g['P'], dM, dMb, g['S1'], g['Rd1'], g['dalpha'], g['alpha'], dtype)
    ms = (2 * n * n + 1,) * 3 + (nx * nx,) * 2 + (n * n + 4 * nx + 17, n * n + 5)
    for j, name in enumerate(st.PART_NAMES):
        out['Q_' + name] = (v[:, j], b[:, j], ms[j])
    ap, ad = 0.83, 0.61
    for name, dname, a, sym in (('X1', dX64[0], ap, True), ('X2', dX64[1], ap, True), ('S1', dS64[0], ap if mut == 'update_ap_on_S1' else ad, True), ('S2', dS64[1], ad, True),
                                ('P', dP64, ad, False)):
        v, b = st.update(g[name], dname, a, dtype, sym)
        out['new_' + name] = (v, b, 3)
    return out


def _outside(val, ref, bound, m):
    return bool(np.any(np.abs(np.asarray(val, LD) - ref) > 4 * sr.gamma(m) * bound))


@pytest.mark.parametrize('condX', [1e1, 1e4, 1e8])
@pytest.mark.parametrize('condS', [1e1, 1e4, 1e8])
@pytest.mark.parametrize('p,nx,mb', [(1, 2, 1), (2, 3, 1), (3, 5, 2), (2, 10, 3)])
def test_fp64_evaluation_stays_inside_the_bounds(p, nx, mb, condS, condX):
    """every inequality of the GPU test with plain fp64 numpy in the place of the kernels, at cond(S), cond(X) up to 1e8"""
    g = _layer_inputs(int(np.log10(condS)) * 1000 + int(np.log10(condX)) * 100 + 10 * p + nx, p, nx, mb, condS, condX)
    got, ref = _layers(g, f64), _layers(g, LD)
    for name, (v, b, m) in ref.items():
        assert not _outside(got[name][0], v, b, m), (name, float(np.max(np.abs(np.asarray(got[name][0], LD) - v) / np.maximum(4 * sr.gamma(m) * b, LD(1e-300)))))
    # the inverse factors: ||L^-1 S L^-T - I||_max <= 4 gamma_{3n} cond_2(S)
    n = nx + mb
    for r in (1, 2):
        for Li, S in ((g[f'L{r}i'], g[f'S{r}']), (g[f'LX{r}i'], g[f'X{r}'])):
            LiL = np.asarray(Li, LD)
            res = np.abs(LiL @ np.asarray(S, LD) @ np.swapaxes(LiL, 1, 2) - np.eye(n)).max(axis=(1, 2))
            assert np.all(res <= 4 * sr.gamma(3 * n) * np.linalg.cond(S)), (r, res)


MUTATIONS = {'dir_ldy_sign_r1': ['dX2'], 'dir_dx_no_half_sum': ['dX1', 'dX2'], 'dir_swap_L_LX': ['W0', 'W1', 'W2', 'W3'], 'dir_corr_other_cone_Si': ['c1', 'c2'],
             'rhs_plus_corrector': ['T1', 'T2'], 'border_bb_sign_dalpha': ['db'], 'update_ap_on_S1': ['new_S1']}


@pytest.mark.parametrize('cond', [1e1, 1e4, 1e8])
@pytest.mark.parametrize('mut', sorted(MUTATIONS))
def test_mutated_reference_leaves_the_bounds(mut, cond):
    """each mutation of a matrix layer, applied to the reference, falls outside 4 gamma_m * bound in the layers it touches and nowhere else"""
    g = _layer_inputs(77 + int(np.log10(cond)), 3, 5, 2, cond, cond)
    ref, bad = _layers(g, LD), _layers(g, LD, mut)
    for name, (v, b, m) in ref.items():
        assert _outside(bad[name][0], v, b, m) == (name in MUTATIONS[mut]), (mut, name)


def test_mutated_control_rules_change_the_step():
    """the two mutations of the control path, on the reference: a step rule with gamma fixed at 0.9, and a pre-test that asks theta = 0.9 instead of (1 / 0.9)(1 + 1e-9)
    -- it would report -1 / 0.9 for a block whose smallest eigenvalue is -1, and the step that follows is longer than the cone allows"""
    eig = np.array([[-0.2, -0.5, -0.3, -0.1], [-0.4, -0.25, -0.6, -0.45]])
    args = (np.ones(2), np.ones(2), 1e-3, 0.0, 0.04, 0.3, 1.7, 0.3, 0.1, -0.05, 1e-4)
    r = st.step_rule(PH_MAIN, eig, *args)
    assert r['ap'] == 1.0 and r['ad'] == 1.0
    eig[0, 1] = -1.0; eig[1, 2] = -1.25
    r, rm = st.step_rule(PH_MAIN, eig, *args), st.step_rule(PH_MAIN, eig, *args, gam_fixed=0.9)
    assert abs(float(r['ap']) - (0.9 + 0.09 * 0.8)) < 1e-15 and abs(float(r['ad']) - (0.9 + 0.09 * 0.8) * 0.8) < 1e-15
    assert abs(float(rm['ap']) - float(r['ap'])) > 1e-3 and abs(float(rm['ad']) - float(r['ad'])) > 1e-3
    # the mutated pre-test: I + 0.9 W is positive definite for lambda_min = -1, so it answers -1 / 0.9 where the eigenvalue is -1
    assert 1.0 + 0.9 * -1.0 > 0.0 and not 1.0 + eig_thresholds(PH_MAIN)[0] * -1.0 > 0.0
    eig_m = eig.copy(); eig_m[0, 1] = -1.0 / 0.9
    rm = st.step_rule(PH_MAIN, eig_m, *args)
    assert float(rm['ap']) < float(r['ap']) - 1e-3
    # centering: damping, no gamma
    rc = st.step_rule(PH_CENTER, eig, *args)
    assert abs(float(rc['ap']) - st.CENTER_DAMP) < 1e-15 and abs(float(rc['ad']) - st.CENTER_DAMP * 0.8) < 1e-15


def test_sigma_rule_exponent_clip_and_floor():
    """k_ctrl_b's rule on the reference: exponent 2, clip to [1e-6, 1], floor at mu_t"""
    eig = -0.5 * np.ones((2, 4))
    a = dict(part_dxs=[-0.02, -0.02], part_xds=[-0.02, -0.02], part_dxds=[0.001, 0.001], sxs=0.09, x0=0.04, s0=0.25, mu=0.1 / 9, mu_t=-1.0, dalpha=-0.01, rd0=0.0, N=9)
    r = st.sigma_rule(eig, **a)
    assert r['ap'] == 1.0 and r['ad'] == 1.0
    rat = float(r['mu_aff']) / a['mu']
    assert 1e-3 < rat < 1.0 and abs(float(r['sigmu']) - rat ** 2 * a['mu']) < 1e-18
    assert abs(float(st.sigma_rule(eig, **a, exponent=3)['sigmu']) - rat ** 3 * a['mu']) < 1e-18
    assert float(st.sigma_rule(eig, **dict(a, mu_t=0.01))['sigmu']) == 0.01                      # floor
    tiny = dict(a, part_dxs=[-0.045, -0.045], part_xds=[-0.0, -0.0], part_dxds=[0.0, 0.0], x0=1e-9, sxs=0.09)
    assert float(st.sigma_rule(eig, **tiny)['sigmu']) == pytest.approx(1e-6 * a['mu'], rel=1e-12)     # lower clip


def _pretest_eligible(shape, generic):
    return 8 < shape[2] + shape[3] <= 32 and not generic


def test_gpu_cases_give_both_kinds_of_pretest_answer():
    """at the reference's own iterates the (shape, K) of the GPU test whose eigenvalues k_eigmin computes (8 < n <= 32, tuned kernels) hold, in pass 2, both blocks
    that the pre-test answers (smallest eigenvalue safely above -1 / theta) and blocks that need the eigenvalue"""
    kinds = set()
    for shape, K, generic in MAIN_CASES:
        if not _pretest_eligible(shape, generic) or shape in LARGE_CASES[1:]:
            continue          # (one large shape is enough here: a dense solve of d = 496 per iteration is slow)
        _, _, _, steps = _walk(shape, K)
        lam = np.linalg.eigvalsh(steps[K - 1][1]['Wm2'])[..., 0]
        th = eig_thresholds(PH_MAIN)[0]
        kinds |= {'bound' if l > -1.0 / th else 'exact' for l in lam.ravel()}
    assert kinds == {'bound', 'exact'}, kinds
    assert all(_pretest_eligible(s, False) for s in CENTER_SHAPES[1:])
