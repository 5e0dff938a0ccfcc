"""tests/t3_reference.py against something that shares no formula with it (no device).

The GPU test (tests/test_gpu_t3_kernels.py) compares the Step 3 kernels of tunempc_amd/csrc/tmpc_t3.h with this reference.  Here the reference is held to
(a) the second-order-cone helpers of the CPU oracle and the defining properties of the Nesterov-Todd scaling, (b) the Schur complement built by brute force from
the constraint operator (HKM for the two LMIs, the linear cone for theta >= 0, NT for the norm cone) and the Newton step of a dense solve of it, (c) the CPU
oracle's path on the cases of the GPU test, (d) bisection for the step lengths into the cone."""
import numpy as np
import pytest

import convexify_oracle as co
import schur_reference as sr
import t3_kernel_cases as tc
import t3_reference as t3

LD = np.longdouble
EPS = sr.EPS


def _cone_point(rng, m1, margin):
    u = rng.standard_normal(m1)
    u[0] = np.linalg.norm(u[1:]) * (1.0 + margin)
    return u


def _rel(a, b):
    a = np.asarray(a.v if isinstance(a, t3.VB) else a, LD); b = np.asarray(b, LD)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- (a) the oracle's helpers, the definition of W
# margin = 1e-3 only: (every quantity but the Mehrotra term, the Mehrotra term); measured 8.04e-14 (det, Jordan division) and 4.48e-13, rounded up one decade
ORACLE_SPREAD = (1e-13, 1e-12)


@pytest.mark.parametrize('m1', [2, 7, 67, 529])
@pytest.mark.parametrize('margin', [1.0, 1e-3])
def test_cone_algebra_against_the_oracle(m1, margin):
    """det, the scaling (beta, v), lambda = W x = W^-1 s, W^-2, the Jordan product and division, the Mehrotra term against the oracle's fp64 helpers: 1e-14 of the
    largest entry at margin = 1 (kappa = 1.67), every quantity.  At margin = 1e-3 (kappa = 1000) the fp64 oracle itself carries kappa eps: ORACLE_SPREAD, the largest
    spreads measured on these seeds rounded up one decade (profiles/t3_kernel_residuals.txt, section 4; tests/tools/t3_kernel_residuals.py)"""
    rng = np.random.default_rng(m1)
    s, x = _cone_point(rng, m1, margin), _cone_point(rng, m1, margin)
    tol, tol_mehrotra = (1e-14, 1e-14) if margin == 1.0 else ORACLE_SPREAD
    assert _rel(t3.det(s), co._soc_det(s)) <= tol
    beta, v = t3.scaling(s, x)
    b64, v64 = co._soc_scaling(s, x)
    assert _rel(beta, b64) <= tol and _rel(v, v64) <= tol
    assert abs(float(beta.v) - b64) <= 4 * sr.gamma(beta.m) * float(beta.b) + tol * b64
    lam = t3.scaled_point(beta, v, x)
    assert _rel(lam, co._soc_W(b64, v64, x)) <= tol and _rel(lam, co._soc_W(b64, v64, s, inverse=True)) <= tol
    assert _rel(t3.W_apply(beta, v, s, inverse=True), lam.v) <= tol
    assert _rel(t3.w2inv(beta, v), co._soc_W2inv(b64, v64)) <= tol
    r = rng.standard_normal(m1)
    assert _rel(t3.jordan(s, r), co._soc_prod(s, r)) <= min(tol, 1e-14)
    assert _rel(t3.jordan_div(s, r), co._soc_div(s, r)) <= tol
    assert _rel(t3.jordan(s, t3.jordan_div(s, r).v), r) <= tol
    dx, ds = rng.standard_normal(m1), rng.standard_normal(m1)
    cor64 = co._soc_W(b64, v64, co._soc_div(co._soc_W(b64, v64, x), co._soc_prod(co._soc_W(b64, v64, dx), co._soc_W(b64, v64, ds, inverse=True))), inverse=True)
    assert _rel(t3.cone_mehrotra(beta, v, lam, dx, ds), cor64) <= tol_mehrotra


@pytest.mark.parametrize('m1', [2, 7, 67])
def test_scaling_is_the_nesterov_todd_point(m1):
    """what defines W without any closed form: W^-2 s = x, W^-2 symmetric positive definite, and W^-2 = 2 u u' - det(u) J for a u in the cone (the quadratic
    representation of a cone point: W is an automorphism of the cone), det(u) = 1 / beta^2; v'Jv = 1"""
    rng = np.random.default_rng(40 + m1)
    s, x = _cone_point(rng, m1, 0.5), _cone_point(rng, m1, 0.2)
    beta, v = t3.scaling(s, x)
    W2 = t3.w2inv(beta, v).v
    tol = 64 * 2.0 ** -64 * m1 * max(t3.kappa(s), t3.kappa(x)) ** 2
    assert np.abs(W2 @ np.asarray(s, LD) - x).max() <= tol * np.abs(x).max()
    assert np.abs(W2 - W2.T).max() == 0 and np.linalg.eigvalsh(np.asarray(W2, float)).min() > 0
    assert abs(t3.det(v.v).v - 1) <= tol
    Jm = np.diag(np.concatenate([[1.0], -np.ones(m1 - 1)])).astype(LD)
    u = W2[:, 0].copy(); u0 = np.sqrt((W2[0, 0] + 1 / (beta.v * beta.v)) / 2); u = u / (2 * u0); u[0] = u0       # from the first column of 2 u u' - det(u) J
    assert u[0] > np.linalg.norm(np.asarray(u[1:], float))
    assert np.abs(2 * np.outer(u, u) - (u[0] * u[0] - u[1:] @ u[1:]) * Jm - W2).max() <= tol * np.abs(W2).max()
    # the general entry (0, 0) is the form the kernel writes for the row of t: Jv_0 = v_0
    assert abs(W2[0, 0] - (1 + 4 * (v.v @ v.v) * v.v[0] ** 2 - 4 * v.v[0] ** 2) / beta.v ** 2) <= tol * W2[0, 0]


def test_starting_point_is_on_the_central_path():
    """k_t3_init: x o s = x0 e and z theta = x0 with s = (t; w c o theta); theta below 1 exactly when x0 n / wr < 1"""
    for p, n, wr in ((2, 3, 0.004), (5, 4, 3.7), (3, 5, 0.31)):
        g = t3.start(p, n, wr)
        m = n * (n + 1) // 2
        s = t3.slack(g['t'].v, np.full(m, g['th'].v), wr, n)
        prod = t3.jordan(g['x'].v, s.v).v
        x0 = LD(1) / (p * n)
        assert abs(prod[0] - x0) <= 1e-17 * t3.kappa(s.v) and np.abs(prod[1:]).max() <= 1e-17 * t3.kappa(s.v)
        assert abs(g['z'].v * g['th'].v - x0) <= 1e-18
        assert (g['th'].v < 1) == (x0 * n / wr < 1)
        assert t3.det(g['x'].v).v > 0 and g['x'].v[0] > 0


# ---------------------------------------------------------------------------------------------------------------- (b) the brute-force Schur complement
def _spd(rng, n, lo=0.3):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return co.symmetrize((Q * rng.uniform(lo, 2.0, n)) @ Q.T)


def _model(seed, p, nx, mb, rows=0):
    rng = np.random.default_rng(seed)
    n = nx + mb; m = n * (n + 1) // 2
    g = dict(p=p, nx=nx, n=n, m=m, d=nx * (nx + 1) // 2, wr=0.51, rows=rows)
    g['V'] = rng.standard_normal((p, nx, n)) / np.sqrt(nx)
    g['Hb'] = np.stack([co.symmetrize(rng.standard_normal((n, n))) for _ in range(p)])
    g['X'] = np.stack([[_spd(rng, n) for _ in range(p)] for _ in range(2)]); g['S'] = np.stack([[_spd(rng, n) for _ in range(p)] for _ in range(2)])
    g['Si'] = np.asarray(np.linalg.inv(g['S']))
    g['th'] = rng.uniform(0.2, 1.5, (p, m)); g['z'] = rng.uniform(0.2, 1.5, (p, m))
    _, _, c, _ = t3.tri(n)
    g['t'] = np.array([np.linalg.norm(g['wr'] * c * g['th'][k]) * rng.uniform(1.2, 2.0) for k in range(p)])
    g['x'] = np.stack([_cone_point(rng, m + 1, 0.3) for _ in range(p)])
    g['G'] = rng.standard_normal((p, rows, n))
    return g


def _brute(g):
    """T_ij = sum over the cones of <A_i, H_c(A_j)> with H_c = sym(X . S^-1) (HKM) for the LMIs, z / theta for the linear cone and W^-2 (from the oracle's dense
    closed form, which t3_reference does not use for the rows) for the norm cone, over the variables (svec P, tau, alpha, phi, theta, t): -> (T, index maps)"""
    p, nx, n, m, d = g['p'], g['nx'], g['n'], g['m'], g['d']
    ta, tb, c, _ = t3.tri(n)
    ia, ib = sr.tri_idx(nx)
    Si = [[sr.LD(1) * np.linalg.inv(np.asarray(g['S'][r, k], LD).astype(float)) for k in range(p)] for r in (0, 1)]
    Si = np.asarray(g['Si'], LD)
    var, img = {}, []          # img[j]: dict cone -> image; cones ('lmi', r, k) matrices, ('lin', k) vector [m], ('soc', k) vector [m + 1]

    def new(key):
        var[key] = len(img); img.append({}); return img[-1]
    for j in range(p):
        for idx in range(d):
            E = np.zeros((p, nx, nx), LD); E[j, ia[idx], ib[idx]] = 1; E[j, ib[idx], ia[idx]] = 1
            dM = sr._calH(np.asarray(g['V'], LD), E, nx, -1)
            A = new(('P', j, idx))
            for k in range(p):
                if dM[k].any():
                    A['lmi', 0, k] = dM[k]; A['lmi', 1, k] = -dM[k]
    A = new(('tau',))
    for k in range(p):
        A['lmi', 1, k] = np.eye(n, dtype=LD)
    A = new(('alpha',))
    for k in range(p):
        A['lmi', 0, k] = np.asarray(g['Hb'][k], LD); A['lmi', 1, k] = -np.asarray(g['Hb'][k], LD)
    for k in range(p):
        for i in range(g['rows']):
            gg = np.outer(np.asarray(g['G'][k, i], LD), np.asarray(g['G'][k, i], LD))
            A = new(('phi', k, i)); A['lmi', 0, k] = gg; A['lmi', 1, k] = -gg
        for e in range(m):
            E = np.zeros((n, n), LD); E[ta[e], tb[e]] = 1; E[tb[e], ta[e]] = 1
            A = new(('th', k, e)); A['lmi', 0, k] = E; A['lmi', 1, k] = -E
            lin = np.zeros(m, LD); lin[e] = 1; A['lin', k] = lin
            soc = np.zeros(m + 1, LD); soc[1 + e] = g['wr'] * c[e]; A['soc', k] = soc
        soc = np.zeros(m + 1, LD); soc[0] = 1
        new(('t', k))['soc', k] = soc
    W2 = {}
    for k in range(p):
        s = t3.slack(g['t'][k], g['th'][k], g['wr'], n).v
        b64, v64 = co._soc_scaling(np.asarray(s, float), g['x'][k])
        W2[k] = np.asarray(co._soc_W2inv(b64, v64), LD)

    def hess(cone, Aj):
        if cone[0] == 'lmi':
            _, r, k = cone
            return sr._sym(np.asarray(g['X'][r, k], LD) @ Aj @ Si[r, k])
        if cone[0] == 'lin':
            return np.asarray(g['z'][cone[1]], LD) / np.asarray(g['th'][cone[1]], LD) * Aj
        return W2[cone[1]] @ Aj
    nv = len(img)
    T = np.zeros((nv, nv), LD)
    for j in range(nv):
        F = {c_: hess(c_, Aj) for c_, Aj in img[j].items()}
        for i in range(nv):
            T[i, j] = sum(np.sum(Ai * F[c_]) for c_, Ai in img[i].items() if c_ in F)
    return T, var


MODELS = [dict(seed=11, p=2, nx=2, mb=1), dict(seed=12, p=1, nx=3, mb=1), dict(seed=13, p=3, nx=2, mb=2, rows=2)]
# Both sides evaluate the same bilinear forms, the reference in np.longdouble; the oracle's W^-2 inside the brute-force matrix is fp64 with the conditioning of the
# cone pair (kappa < 10 for the margins of _model): 1e3 EPS of the largest entry.  A mutation changes an entry by its own size.
TOL = 1e3 * EPS


@pytest.mark.parametrize('mdl', MODELS, ids=lambda m: f"seed{m['seed']}-p{m['p']}")
def test_rows_equal_the_brute_force_schur_matrix(mdl):
    """b, a (a + b at p = 1), the theta-theta block, the row of t, the block between theta and the multipliers of G / C, and c_tau, c_alpha from Psi, Phi equal the
    entries of the matrix built from the constraint operator alone; the rows reach P_k, P_k+1, tau, alpha and their own stage only; the matrix is symmetric"""
    g = _model(**mdl)
    T, var = _brute(g)
    p, nx, n, m, d = g['p'], g['nx'], g['n'], g['m'], g['d']
    scale = np.abs(T).max()
    assert np.abs(T - T.T).max() <= TOL * scale
    for k in range(p):
        kn = (k + 1) % p
        s = t3.slack(g['t'][k], g['th'][k], g['wr'], n)
        beta, v = t3.scaling(s, g['x'][k])
        R = t3.schur_rows(g['X'][:, k], g['Si'][:, k], g['V'][k], beta.v, v.v, g['th'][k], g['z'][k], g['wr'], nx)
        th = [var['th', k, e] for e in range(m)]; tt = var['t', k]
        pk = [var['P', k, i] for i in range(d)]; pkn = [var['P', kn, i] for i in range(d)]
        diffs = [R['H'].v - T[np.ix_(th, th)], R['trow'].v - T[tt, th + [tt]]]
        if p == 1:
            diffs.append(R['a'].v + R['b'].v - T[np.ix_(th, pk)])
        else:
            diffs += [R['a'].v - T[np.ix_(th, pk)], R['b'].v - T[np.ix_(th, pkn)]]
        assert not T[tt, pk + pkn + [var['tau',], var['alpha',]]].any()
        others = [j for key, j in var.items() if key[0] in ('P', 'phi', 'th', 't') and key[1] not in (k, kn) or key[0] in ('phi', 'th', 't') and key[1] != k]
        assert not T[np.ix_(th + [tt], others)].any()
        if g['rows']:
            X, Si = np.asarray(g['X'][:, k], LD), np.asarray(g['Si'][:, k], LD)
            w = np.stack([np.asarray(g['G'][k], LD) @ X[r] for r in (0, 1)]); u = np.stack([np.asarray(g['G'][k], LD) @ Si[r] for r in (0, 1)])
            diffs.append(t3.cross(w, u, n).v - T[np.ix_(th, [var['phi', k, i] for i in range(g['rows'])])])
        ta, tb, c, we = t3.tri(n)
        X, Si, Hb = np.asarray(g['X'][:, k], LD), np.asarray(g['Si'][:, k], LD), np.asarray(g['Hb'][k], LD)
        Psi = sr._sym(X[1] @ Si[1]); Phi = sr._sym(X[0] @ Hb @ Si[0]) + sr._sym(X[1] @ Hb @ Si[1])
        _, ct, ca = t3.gather_rows(np.zeros((n, n)), np.zeros((n, n)), g['th'][k], None, np.zeros(m + 1), np.zeros(m + 1), Psi, Phi, 0.0, g['wr'], n)
        diffs += [ct - T[th, var['tau',]], ca - T[th, var['alpha',]]]
        assert max(float(np.abs(x).max()) for x in diffs) <= TOL * scale, [float(np.abs(x).max() / scale) for x in diffs]


def test_newton_step_of_the_cones():
    """the directions of k_t3_dir solve the linearised complementarity of both cones for any (dth, dt): z dth + th dz = sig - th z - th cth, and
    W-scaled: lambda o (W dx + W^-1 ds) = sig e - lambda o lambda - (W dx_aff) o (W^-1 ds_aff) with g of k_t3_rhs and the Mehrotra term of pass 1"""
    rng = np.random.default_rng(5)
    g = _model(21, 1, 2, 2)
    n, m, wr = g['n'], g['m'], g['wr']
    th, z, t, x = g['th'][0], g['z'][0], g['t'][0], g['x'][0]
    s = t3.slack(t, th, wr, n).v
    beta, v = (a.v for a in t3.scaling(s, x))
    lam = t3.scaled_point(beta, v, x).v
    e = np.zeros(m + 1, LD); e[0] = 1
    # pass 1
    dth1, dt1 = rng.standard_normal(m), rng.standard_normal()
    ds1 = t3.cone_ds(dt1, dth1, wr, n).v
    g1 = t3.rhs_g(t, th, x, None, 0.0, wr, n).v
    dx1 = t3.cone_dx(g1, beta, v, ds1).v
    lhs = t3.jordan(lam, t3.W_apply(beta, v, dx1).v + t3.W_apply(beta, v, ds1, inverse=True).v).v
    assert np.abs(lhs + t3.jordan(lam, lam).v).max() <= 1e-15 * t3.kappa(s) * t3.kappa(x)
    cq = t3.cone_mehrotra(beta, v, lam, dx1, ds1).v
    dz1 = t3.dual_direction(th, z, dth1, 0.0, None).v
    cth = t3.mehrotra_theta(dz1, dth1, th).v
    th, z = np.asarray(th, LD), np.asarray(z, LD)
    assert np.abs(z * dth1 + th * dz1 + th * z).max() <= 1e-17
    # pass 2, main phase
    sig = 0.07
    dth, dt = rng.standard_normal(m), rng.standard_normal()
    ds = t3.cone_ds(dt, dth, wr, n).v
    g2 = t3.rhs_g(t, th, x, cq, sig, wr, n).v
    dx = t3.cone_dx(g2, beta, v, ds).v
    lhs = t3.jordan(lam, t3.W_apply(beta, v, dx).v + t3.W_apply(beta, v, ds, inverse=True).v).v
    rhs = sig * e - t3.jordan(lam, lam).v - t3.jordan(t3.W_apply(beta, v, dx1).v, t3.W_apply(beta, v, ds1, inverse=True).v).v
    assert np.abs(lhs - rhs).max() <= 1e-15 * t3.kappa(s) * t3.kappa(x) * max(1.0, float(np.abs(rhs).max()))
    dz = t3.dual_direction(th, z, dth, sig, cth).v
    assert np.abs(z * dth + th * dz - (sig - th * z - dz1 * dth1)).max() <= 1e-16


# ---------------------------------------------------------------------------------------------------------------- (c) the cases of the GPU test on the oracle
@pytest.mark.parametrize('case', tc.ALL_SHAPES, ids=lambda c: 'nb{}-p{}-nx{}-mb{}-ng{}-nc{}'.format(*c[:6]))
def test_cases_are_in_the_main_phase_at_K(case):
    """every member the solver iterates on: indefinite H; the oracle is still in the main phase at every K of the case; no pivot is frozen on the way (shift = 0);
    for K >= 2 T has left its starting value by more than 1e-2 relative; some case starts theta below 1"""
    prob = tc.make_problem(case)
    Ks = tc.case_K(case)
    nb, p, nx, mb = case[:4]
    for b in range(nb):
        lo = min(np.linalg.eigvalsh(prob['H'][b, k]).min() for k in range(p))
        if b not in tc.solved_members(case):
            assert lo > 0
            continue
        assert lo < 0
        kw = tc.oracle_rows(case, b, prob)
        args = (prob['A'][b], prob['B'][b], prob['H'][b])
        trace = []
        r = co.sdp_step1(*args, dict(max_iter=max(Ks)), trace=trace, **kw)
        assert len(trace) >= max(Ks) and all(t['phase'] == 0 for t in trace[:max(Ks)]) and r['shift'] == 0.0
        start = co.sdp_step1(*args, dict(max_iter=0), **kw)['T']
        for K in Ks:
            if K >= 2:
                now = co.sdp_step1(*args, dict(max_iter=K - 1), **kw)['T']
                assert np.linalg.norm(now - start) > 1e-2 * np.linalg.norm(now), (K, 'T still at its starting value')


def test_some_case_starts_theta_below_one():
    hits = []
    for case in tc.ALL_SHAPES:
        prob = tc.make_problem(case)
        s, sbeta = co.auto_scaling(prob['H'][tc.solved_members(case)[0]])
        hits.append(1.0 / case[1] / (case[7] * sbeta / s) < 1.0)
    assert any(hits) and not all(hits)


# ---------------------------------------------------------------------------------------------------------------- (d) step lengths against bisection
def step_pairs(m1, seed=0):
    """the pairs (u, du) of tests/test_gpu_t3_kernels.py section c: -> [(name, u, du)]"""
    rng = np.random.default_rng(1000 * m1 + seed)
    out = []
    base = _cone_point(rng, m1, 0.5)
    e1 = np.zeros(m1); e1[0] = 1.0; e1[1] = 1.0
    inner = _cone_point(rng, m1, 0.3)
    out.append(('du inside the cone', base, inner))
    out.append(('du on the boundary, bq > 0', np.concatenate([[2.0], [0.5], np.zeros(m1 - 2)]), e1))
    nb_ = e1.copy(); nb_[0] = -1.0
    out.append(('du on the boundary of -Q, bq < 0', np.concatenate([[2.0], [0.5], np.zeros(m1 - 2)]), nb_))
    out.append(('du in -Q', base, -inner))
    sp = rng.standard_normal(m1); sp[0] = -0.1 * np.linalg.norm(sp[1:])
    out.append(('du0 < 0 outside both cones', base, sp))
    near = _cone_point(rng, m1, 1e-8)
    out.append(('u near the boundary', near, rng.standard_normal(m1)))
    # du within 1e-6 .. 1e-15 of the boundary of -Q: a -> 0+ carries few digits; the exit c / (-bq + sqrt(disc)) does not depend on them
    for rel in (1e-6, 1e-10, 1e-13, 1e-15):
        d = rng.standard_normal(m1); d[1:] /= np.linalg.norm(d[1:]); d[0] = -(1.0 + rel)
        u = np.concatenate([[2.0], 0.5 * d[1:]])
        out.append((f'du {rel:g} inside -Q, along u1', u, d))
        out.append((f'du {rel:g} inside -Q, against u1', u, np.concatenate([d[:1], -d[1:]])))
    for i in range(6):
        out.append((f'random {i}', _cone_point(rng, m1, rng.uniform(0.01, 2.0)), rng.standard_normal(m1)))
    return out


@pytest.mark.parametrize('m1', [2, 64, 65, 67, 529])
def test_step_lengths_against_bisection(m1):
    """the fp64 restatement of soc_step_eig: unbounded exactly when the ray stays inside; else th = -1/eig is a root of det(u + th du) (residual in units of eps,
    the constant the GPU test derives its own from), 0.999 th is strictly inside, and no smaller positive root exists (bisection)"""
    worst = 0.0
    for name, u, du in step_pairs(m1):
        eig = t3.soc_step_eig64(u, du)
        ref = t3.soc_step_bisect(u, du)
        if ref == np.inf:
            assert eig == 0.0, name
            continue
        assert eig < 0.0, name
        th = -1.0 / eig
        assert t3.soc_inside(u, du, 0.999 * th), name
        assert abs(th - ref) <= 1e-6 * ref, (name, th, ref)
        worst = max(worst, t3.soc_root_residual(u, du, th) / EPS)
    assert worst < 1e3, worst


def test_update_with_a_zero_step_is_the_identity():
    """the reference's update with a = 0 returns the state bit for bit, whatever the direction holds: what k_t3_update's guard `ap == 0 && ad == 0` (a discarded
    direction) must leave.  No case reaches the guard on the device: the solver discards a direction only after a failed factorisation."""
    x = np.array([1.5, -0.25, 3.0])
    assert np.array_equal(np.asarray(t3.update(x, np.array([7.0, -2.0, 1e300]), 0.0).v, float), x)
