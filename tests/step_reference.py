"""Plain numpy reference of the second half of an interior-point iteration -- what turns a solved block system into the next iterate -- one function per layer,
for tests/test_step_reference_cpu.py and tests/test_gpu_step_kernels.py.  No device, no oracle import.  Same conventions as tests/schur_reference.py, whose gamma,
_calH, schur_blocks and rhs_columns it reuses: every function takes the INPUTS OF ITS OWN LAYER and returns (value, bound), the value in `dtype` (np.longdouble) and
the bound as the same formula on absolute values with every subtraction turned into an addition; a kernel that forms an entry in m nested fp64 operations errs by at
most gamma_m * bound.  Where a layer consumes a quantity the device never stores (dM, Ldy, the border right-hand side), the reference forms it from the stored
inputs as the kernel does and its bound carries that quantity's own bound, so the operation counts add.

The rules, each stated once, with the kernel line it restates (tunempc_amd/csrc):
  T_r      = sigma mu S_r^-1 - sym(X_r Rd_r S_r^-1) - c_r, c_r only in pass 2 of the main phase      stage_rhs_body: `double t = sig * sSi[..] - 0.5 * (t1[..] + t1[..]); if (use_corr) t -= cg[e];`
  Q_TRT2   = tr T_2, Q_HBG = <Hb, T_1 - T_2> per stage                                                 stage_rhs_body: `gr[q] -= t; if (i == j) trt2 += t;`, `hbg = fma(Hbg[e], gr[q], hbg)`
  SB       = [[btt, bta], [bta, baa]] - U' TU                                                          solve_border_body: `pr[P_SB00] = pr[P_BTT] - s00; ...`
  rb       = [(sum Q_TRT2 - 1) - u_tau' z, (sum Q_HBG + t0) - u_alpha' z], t0 = sigma mu / s0 - x0 rd0 / s0 - corr0       `const double rb0 = (trt2 - 1.0) - u0, rb1 = (hbg + t0) - u1;`
  dtau     = (SB11 rb0 - SB01 rb1) / det, dalpha = (SB00 rb1 - SB01 rb0) / det, det = SB00 SB11 - SB01^2                    `const double dtau = (c * rb0 - bb * rb1) / det, ...`
  dP_k     = smat(z_k - TU_k [dtau, dalpha]'), svec index over the row-major upper triangle           `const double v = Z[vi] - TU[vi * 2] * dtau - TU[vi * 2 + 1] * dalpha;`
  dM_k     = dalpha Hb_k + V_k' dP_{k+1} V_k - E' dP_k E                                               stage_dir_body: `build_M<NT>(sM, ..., dPk, ..., dalpha, ...)`
  Ldy_1    = dM, Ldy_2 = dtau I - dM;  dS_r = Ldy_r + Rd_r                                            `const double ldy = (r == 0) ? dm_ : ((i == j ? dtau : 0.0) - dm_); const double ds = ldy + Rdg[e];`
  dX_r     = T_r - X_r - sym(X_r Ldy_r S_r^-1)                                                         `const double dx = Tg[e] - sX[..] - 0.5 * (t1[..] + t1[..]);`
  W[2r]    = L_r^-1 dS_r L_r^-T (dual), W[2r+1] = LX_r^-1 dX_r LX_r^-T (primal), symmetrised          `s2g_sym<NT>(w.Wm + ((size_t)sid * 4 + 2 * r) * nn, t1, n, lane);` and `... + 2 * r + 1 ...`
  c_r      = sym(dX_r dS_r S_r^-1), pass 1 only                                                        `if (pass == 1) { ... s2g_sym<NT>((r ? w.c2 : w.c1) + ..., t1, n, lane); }`
  partial sums per stage: <dX,S>, <X,dS>, <dX,dS> over both cones, |dP_k|^2, |P_k|^2, |dM - (dalpha/alpha) M|^2, |M|^2 with M = S_1 + Rd_1 + I       `q[Q_DXS] = dxs; ...`
  raw steps: a_p = -1 / min eig (primal slots), 1e300 if >= 0; then min(a_p, -x0 / dx0) if dx0 < 0; a_d likewise from the dual slots, s0, ds0        tmpc_schur.h raw_steps
  sigma    = clip((mu_aff / mu)^2, 1e-6, 1), sigma mu floored at mu_t once mu_t > 0; corr0 = dx0 ds0 / s0 with the predictor's dx0 = -x0 - x0 ds0 / s0       ctrl_b_body
  step     main: gamma = 0.9 + 0.09 min(min(a_p, a_d), 1), a = min(1, gamma a); centering: a = min(1, CENTER_DAMP a);
           ds0 = dalpha + rd0, dx0 = sigma mu / s0 - x0 - x0 ds0 / s0 - corr0; x0 += a_p dx0, s0 += a_d ds0, tau += a_d dtau, alpha += a_d dalpha;
           P_STEPN = sqrt(sum Q_DH2 / sum Q_M2), P_RAWSTEP = min of the raw steps                                                                       ctrl_c_body
  update   X_r <- sym(X_r + a_p dX_r), S_r <- sym(S_r + a_d dS_r), P <- P + a_d dP                    update_body: `0.5 * ((w.X1[o + e] + ap * w.dX1[o + e]) + (w.X1[o + et] + ap * w.dX1[o + et]))`

Shapes: one problem at a time, stage-stacked [p, ...]; n = nx + mb, d = nx (nx + 1) / 2."""
import numpy as np

import schur_reference as sr

LD = sr.LD
CENTER_DAMP = 0.95          # TMPC_CENTER_DAMP of csrc/tmpc_common.h
ALPHA_MIN = 1e-8            # ALPHA_MIN of csrc/tmpc_common.h
_t, _sym = sr._t, sr._sym


def _a(dtype, *arrs):
    return [np.asarray(x, dtype) for x in arrs]


# ---------------------------------------------------------------------------------------------------------------- pass-2 right-hand side
def corrector_T(X, Rd, Si, sigmu, c=None, dtype=LD):
    """T_r = sigma mu S_r^-1 - sym(X_r Rd_r S_r^-1) - c_r (c = None: no corrector).   -> (T, bound)"""
    X, Rd, Si = _a(dtype, X, Rd, Si)
    sg = dtype(sigmu)
    T = sg * Si - _sym(X @ Rd @ Si)
    B = abs(sg) * np.abs(Si) + _sym(np.abs(X) @ np.abs(Rd) @ np.abs(Si))
    if c is not None:
        c = np.asarray(c, dtype)
        T = T - c; B = B + np.abs(c)
    return T, B


def rhs_partials(T1, T2, Hb, dtype=LD):
    """per stage: Q_TRT2 = tr T2, Q_HBG = <Hb, T1 - T2>.   -> ([p, 2], bound)"""
    T1, T2, Hb = _a(dtype, T1, T2, Hb)
    tr = np.trace(T2, axis1=-2, axis2=-1); trb = np.trace(np.abs(T2), axis1=-2, axis2=-1)
    hbg = np.sum(Hb * (T1 - T2), axis=(-2, -1)); hbb = np.sum(np.abs(Hb) * (np.abs(T1) + np.abs(T2)), axis=(-2, -1))
    return np.stack([tr, hbg], axis=-1), np.stack([trb, hbb], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- border solve
def border_matrix(btt, bta, baa, U, TU, dtype=LD):
    """SB00, SB01, SB11 = [btt, bta, baa] - [u_tau' tu_tau, u_tau' tu_alpha, u_alpha' tu_alpha]; U, TU [p, dp, 2].   -> ([3], bound)"""
    U, TU = _a(dtype, U, TU)
    b = np.array([btt, bta, baa], dtype)
    s = np.array([np.sum(U[..., 0] * TU[..., 0]), np.sum(U[..., 0] * TU[..., 1]), np.sum(U[..., 1] * TU[..., 1])], dtype)
    Ua, Ta = np.abs(U), np.abs(TU)
    sa = np.array([np.sum(Ua[..., 0] * Ta[..., 0]), np.sum(Ua[..., 0] * Ta[..., 1]), np.sum(Ua[..., 1] * Ta[..., 1])], dtype)
    return b - s, np.abs(b) + sa


def border_rhs(trt2, hbg, Z, U, sigmu, corr0, s0, x0, rd0, dtype=LD):
    """rb = [(sum trt2 - 1) - u_tau' z, (sum hbg + t0) - u_alpha' z], t0 = sigma mu / s0 - x0 rd0 / s0 - corr0.   -> ([2], bound)"""
    trt2, hbg, Z, U = _a(dtype, trt2, hbg, Z, U)
    sg, c0, s0, x0, rd0 = (dtype(v) for v in (sigmu, corr0, s0, x0, rd0))
    t0 = sg / s0 - x0 * rd0 / s0 - c0
    t0b = abs(sg / s0) + abs(x0 * rd0 / s0) + abs(c0)
    rb = np.array([(trt2.sum() - 1) - np.sum(U[..., 0] * Z), (hbg.sum() + t0) - np.sum(U[..., 1] * Z)], dtype)
    rbb = np.array([np.abs(trt2).sum() + 1 + np.sum(np.abs(U[..., 0] * Z)), np.abs(hbg).sum() + t0b + np.sum(np.abs(U[..., 1] * Z))], dtype)
    return rb, rbb


def border_solution(SB, rb, rbb, dtype=LD):
    """(dtau, dalpha) by Cramer's rule.  bound of a quotient N / det: Nabs / |det| + |N| detabs / det^2 (the roundings of numerator and denominator).   -> ([2], bound)"""
    a, bb, c = (dtype(v) for v in SB)
    rb, rbb = _a(dtype, rb, rbb)
    det = a * c - bb * bb; deta = abs(a * c) + bb * bb
    N = np.array([c * rb[0] - bb * rb[1], a * rb[1] - bb * rb[0]], dtype)
    Na = np.array([abs(c) * rbb[0] + abs(bb) * rbb[1], abs(a) * rbb[1] + abs(bb) * rbb[0]], dtype)
    return N / det, Na / abs(det) + np.abs(N) * deta / (det * det)


def direction_P(Z, TU, dtau, dalpha, nx, dtype=LD):
    """dP_k = smat(z_k - tu_tau dtau - tu_alpha dalpha) over the first d entries of the padded vectors [p, dp].   -> ([p, nx, nx], bound)"""
    Z, TU = _a(dtype, Z, TU)
    ia, ib = sr.tri_idx(nx)
    d = len(ia)
    dt, da = dtype(dtau), dtype(dalpha)
    v = Z[:, :d] - TU[:, :d, 0] * dt - TU[:, :d, 1] * da
    vb = np.abs(Z[:, :d]) + np.abs(TU[:, :d, 0] * dt) + np.abs(TU[:, :d, 1] * da)
    out = np.zeros((Z.shape[0], nx, nx), dtype); bnd = np.zeros_like(out)
    out[:, ia, ib] = v; out[:, ib, ia] = v; bnd[:, ia, ib] = vb; bnd[:, ib, ia] = vb
    return out, bnd


# ---------------------------------------------------------------------------------------------------------------- directions
def direction_M(dP, dalpha, Hb, V, nx, dtype=LD):
    """dM = dalpha Hb + calH(dP).   -> ([p, n, n], bound)"""
    dP, Hb, V = _a(dtype, dP, Hb, V)
    da = dtype(dalpha)
    return da * Hb + sr._calH(V, dP, nx, -1), abs(da) * np.abs(Hb) + sr._calH(np.abs(V), np.abs(dP), nx, 1)


def linear_parts(dM, dMb, dtau, dtype=LD):
    """Ldy_1 = dM, Ldy_2 = dtau I - dM.   -> ((Ldy1, Ldy2), (bound1, bound2))"""
    I = np.eye(dM.shape[-1], dtype=dtype)
    return (dM, dtype(dtau) * I - dM), (dMb, abs(dtype(dtau)) * I + dMb)


def direction_S(Ldy, Ldyb, Rd, dtype=LD):
    """dS_r = Ldy_r + Rd_r"""
    Rd = np.asarray(Rd, dtype)
    return Ldy + Rd, Ldyb + np.abs(Rd)


def direction_X(T, X, Ldy, Ldyb, Si, dtype=LD, half_sum=True, sign=1):
    """dX_r = T_r - X_r - sym(X_r Ldy_r S_r^-1).  (half_sum / sign: the mutations of tests/test_step_reference_cpu.py.)"""
    T, X, Si = _a(dtype, T, X, Si)
    t1 = X @ (sign * Ldy) @ Si
    return T - X - (_sym(t1) if half_sum else t1), np.abs(T) + np.abs(X) + _sym(np.abs(X) @ Ldyb @ np.abs(Si))


def step_matrix(Li, dS, dtype=LD):
    """W = sym(L^-1 dS L^-T)"""
    Li, dS = _a(dtype, Li, dS)
    return _sym(Li @ dS @ _t(Li)), _sym(np.abs(Li) @ np.abs(dS) @ np.abs(_t(Li)))


def corrector_term(dX, dS, Si, dtype=LD):
    """c_r = sym(dX_r dS_r S_r^-1)"""
    dX, dS, Si = _a(dtype, dX, dS, Si)
    return _sym(dX @ dS @ Si), _sym(np.abs(dX) @ np.abs(dS) @ np.abs(Si))


PART_NAMES = ('DXS', 'XDS', 'DXDS', 'DP2', 'P2', 'DH2', 'M2')


def partial_sums(dX, dS, X, S, dP, P, dM, dMb, S1, Rd1, dalpha, alpha, dtype=LD):
    """The seven per-stage sums of stage_dir in PART_NAMES order; dX, dS, X, S: pairs (cone 1, cone 2).   -> ([p, 7], bound)"""
    ax = (-2, -1)
    dX, dS, X, S = (_a(dtype, *q) for q in (dX, dS, X, S))
    dP, P, S1, Rd1 = _a(dtype, dP, P, S1, Rd1)
    ra = dtype(dalpha) / dtype(alpha)
    I = np.eye(S1.shape[-1], dtype=dtype)
    M = S1 + Rd1 + I; Mb = np.abs(S1) + np.abs(Rd1) + I
    dh = dM - ra * M; dhb = dMb + abs(ra) * Mb
    val = [sum(np.sum(dX[r] * S[r], axis=ax) for r in (0, 1)), sum(np.sum(X[r] * dS[r], axis=ax) for r in (0, 1)), sum(np.sum(dX[r] * dS[r], axis=ax) for r in (0, 1)),
           np.sum(dP * dP, axis=ax), np.sum(P * P, axis=ax), np.sum(dh * dh, axis=ax), np.sum(M * M, axis=ax)]
    bnd = [sum(np.sum(np.abs(dX[r] * S[r]), axis=ax) for r in (0, 1)), sum(np.sum(np.abs(X[r] * dS[r]), axis=ax) for r in (0, 1)),
           sum(np.sum(np.abs(dX[r] * dS[r]), axis=ax) for r in (0, 1)), val[3], val[4], np.sum(dhb * dhb, axis=ax), np.sum(Mb * Mb, axis=ax)]
    return np.stack(val, axis=-1), np.stack(bnd, axis=-1)


# ---------------------------------------------------------------------------------------------------------------- control rules
def raw_steps(minx, mins, dx0, ds0, x0, s0, dtype=LD):
    """(a_p, a_d) before damping and clipping; one division each"""
    minx, mins, dx0, ds0, x0, s0 = (dtype(v) for v in (minx, mins, dx0, ds0, x0, s0))
    big = dtype(1e300)
    ap = big if minx >= 0 else -1 / minx
    ad = big if mins >= 0 else -1 / mins
    if dx0 < 0:
        ap = min(ap, -x0 / dx0)
    if ds0 < 0:
        ad = min(ad, -s0 / ds0)
    return ap, ad


def eig_minima(eigmin):
    """[p, 4] -> (minx, mins): the primal minimum over slots 1, 3 and the dual one over slots 0, 2 (emin of tmpc_schur.h)"""
    e = np.asarray(eigmin)
    return min(e[:, 1].min(), e[:, 3].min()), min(e[:, 0].min(), e[:, 2].min())


def sigma_rule(eigmin, part_dxs, part_xds, part_dxds, sxs, x0, s0, mu, mu_t, dalpha, rd0, N, dtype=LD, exponent=2):
    """k_ctrl_b: -> dict(sigmu, corr0, and their bounds sigmu_b, corr0_b, the clipped affine steps ap, ad)"""
    x0, s0, mu, dalpha, rd0, sxs = (dtype(v) for v in (x0, s0, mu, dalpha, rd0, sxs))
    dxs, xds, dxds = (np.asarray(v, dtype).sum() for v in (part_dxs, part_xds, part_dxds))
    dxsb, xdsb, dxdsb = (np.abs(np.asarray(v, dtype)).sum() for v in (part_dxs, part_xds, part_dxds))
    minx, mins = eig_minima(eigmin)
    ds0 = dalpha + rd0; ds0b = abs(dalpha) + abs(rd0)
    dx0 = -x0 - x0 * ds0 / s0; dx0b = x0 + x0 * ds0b / s0
    ap, ad = raw_steps(minx, mins, dx0, ds0, x0, s0, dtype)
    ap = min(dtype(1), ap); ad = min(dtype(1), ad)
    ma = (sxs + ap * dxs + ad * xds + ap * ad * dxds + (x0 + ap * dx0) * (s0 + ad * ds0)) / N
    mab = (abs(sxs) + ap * dxsb + ad * xdsb + ap * ad * dxdsb + (x0 + ap * dx0b) * (s0 + ad * ds0b)) / N
    rat = ma / mu
    sigma = min(max(rat ** exponent, dtype(1e-6)), dtype(1))
    sig_mu = sigma * mu
    if mu_t > 0:
        sig_mu = max(sig_mu, dtype(mu_t))
    # d(rat^2 mu) = 2 rat mu d(rat): the bound of sigma mu carries the cancellation of mu_aff twice, plus its own value
    sig_b = 2 * abs(rat) * mab + abs(sig_mu)
    return dict(sigmu=sig_mu, sigmu_b=sig_b, corr0=dx0 * ds0 / s0, corr0_b=dx0b * ds0b / s0, ap=ap, ad=ad, mu_aff=ma)


def step_rule(phase, eigmin, part_dh2, part_m2, sigmu, corr0, x0, s0, tau, alpha, dtau, dalpha, rd0, dtype=LD, gam_fixed=None):
    """k_ctrl_c on a step that is taken (no frozen pivot, finite): -> dict(ap, ad, rawstep, stepn, x0, s0, tau, alpha, dx0, ds0 and the bounds x0_b, s0_b, tau_b, alpha_b)"""
    sigmu, corr0, x0, s0, tau, alpha, dtau, dalpha, rd0 = (dtype(v) for v in (sigmu, corr0, x0, s0, tau, alpha, dtau, dalpha, rd0))
    minx, mins = eig_minima(eigmin)
    ds0 = dalpha + rd0; ds0b = abs(dalpha) + abs(rd0)
    dx0 = sigmu / s0 - x0 - x0 * ds0 / s0 - corr0; dx0b = abs(sigmu / s0) + x0 + x0 * ds0b / s0 + abs(corr0)
    rp, rd = raw_steps(minx, mins, dx0, ds0, x0, s0, dtype)
    raw = min(rp, rd)
    one = dtype(1)
    if phase == 0:
        gam = dtype(0.9) + dtype(0.09) * min(raw, one) if gam_fixed is None else dtype(gam_fixed)
        ap = min(one, gam * rp); ad = min(one, gam * rd)
    else:
        ap = min(one, dtype(CENTER_DAMP) * rp); ad = min(one, dtype(CENTER_DAMP) * rd)
    stepn = np.sqrt(np.asarray(part_dh2, dtype).sum() / np.asarray(part_m2, dtype).sum())
    return dict(ap=ap, ad=ad, rawstep=raw, stepn=stepn, dx0=dx0, ds0=ds0, dx0_b=dx0b, ds0_b=ds0b, x0=x0 + ap * dx0, s0=s0 + ad * ds0, tau=tau + ad * dtau, alpha=alpha + ad * dalpha,
                x0_b=x0 + ap * dx0b, s0_b=s0 + ad * ds0b, tau_b=abs(tau) + abs(ad * dtau), alpha_b=abs(alpha) + abs(ad * dalpha))


def update(X, dX, a, dtype=LD, symmetric=True):
    """sym(X + a dX) (P: symmetric = False, dP is symmetric as built)"""
    X, dX = _a(dtype, X, dX)
    a = dtype(a)
    v = X + a * dX; b = np.abs(X) + np.abs(a * dX)
    return (_sym(v), _sym(b)) if symmetric else (v, b)


# ---------------------------------------------------------------------------------------------------------------- one whole iteration, dense
def _chol_parts(S):
    L = np.linalg.cholesky(S)
    Li = np.stack([np.linalg.solve(L[k], np.eye(S.shape[-1])) for k in range(S.shape[0])])
    return Li, _sym(_t(Li) @ Li)


def dense_schur(D, C):
    """the block-cyclic tridiagonal T [p d, p d] from D_k = T[P_k, P_k] and C_k = T[P_k, P_{k+1 mod p}]"""
    p, d, _ = D.shape
    T = np.zeros((p * d, p * d), D.dtype)
    for k in range(p):
        kn = (k + 1) % p
        T[k * d:(k + 1) * d, k * d:(k + 1) * d] += D[k]
        T[k * d:(k + 1) * d, kn * d:(kn + 1) * d] += C[k]
        T[kn * d:(kn + 1) * d, k * d:(k + 1) * d] += C[k].T
    return T


def primal_residuals(X1, X2, x0, Hb, V, nx, dtype=LD):
    """the three primal equations of k_ctrl_a, linear in the iterate: r_tau = 1 - sum tr X2, r_alpha = -<Hb, X1 - X2> - x0, r_P = -svec_grad(calH*(X1 - X2)).
    -> (r_tau, r_alpha, r_P [p, d], scale): scale = the absolute-value form of the same sums (what 'relative' refers to)"""
    X1, X2, Hb, V = _a(dtype, X1, X2, Hb, V)
    ia, ib = sr.tri_idx(nx)
    Y = X1 - X2
    r_tau = 1 - np.trace(X2, axis1=-2, axis2=-1).sum()
    r_alpha = -np.sum(Hb * Y) - dtype(x0)
    r_P = -sr._svec_grad(sr._calH_adj(V, Y, nx, -1), ia, ib)
    Ya = np.abs(X1) + np.abs(X2)
    scale = max(1 + np.trace(np.abs(X2), axis1=-2, axis2=-1).sum(), np.sum(np.abs(Hb) * Ya) + abs(dtype(x0)), sr._svec_grad(sr._calH_adj(np.abs(V), Ya, nx, 1), ia, ib).max())
    return r_tau, r_alpha, r_P, scale


def newton_iteration(it, mutate=None):
    """One whole iteration in fp64 from the iterate `it` (dict: X1, X2, S1, S2, P, V, Hb, tau, alpha, x0, s0, mu_t (None or <= 0: not set yet), phase (0 main, 1
    centering), tol): the bordered system assembled densely (sr.schur_blocks, sr.rhs_columns_at_iterate), one LAPACK solve per pass, then the layer functions
    above.  -> (next iterate, info: mu, pinf, dinf, sigmu, ap, ad, rawstep, the pass-2 direction, the step-length matrices Wm [p, 4, n, n] of both passes)."""
    f = np.float64
    X1, X2, S1, S2, P, V, Hb = (np.asarray(it[k], f) for k in ('X1', 'X2', 'S1', 'S2', 'P', 'V', 'Hb'))
    tau, alpha, x0, s0 = (float(it[k]) for k in ('tau', 'alpha', 'x0', 's0'))
    phase = int(it.get('phase', 0))
    mu_t = it.get('mu_t') or -1.0
    p, nx, n = V.shape
    d = nx * (nx + 1) // 2
    N = 2 * p * n + 1
    ia, ib = sr.tri_idx(nx)
    L1i, S1i = _chol_parts(S1); L2i, S2i = _chol_parts(S2)
    LX1i, _ = _chol_parts(X1); LX2i, _ = _chol_parts(X2)
    Rd1, Rd2, _, _ = sr.dual_residuals(P, tau, alpha, Hb, V, S1, S2, nx, f)
    rd0 = (alpha - ALPHA_MIN) - s0
    sxs = np.sum(X1 * S1) + np.sum(X2 * S2)
    mu = (sxs + x0 * s0) / N
    r_tau, r_alpha, r_P, _ = primal_residuals(X1, X2, x0, Hb, V, nx, f)
    pinf = np.sqrt(r_tau ** 2 + r_alpha ** 2 + np.sum(r_P ** 2)) / 2.0
    dinf = np.sqrt(np.sum(Rd1 ** 2) + np.sum(Rd2 ** 2) + rd0 ** 2) / (1.0 + np.sqrt(np.sum(S1 ** 2) + np.sum(S2 ** 2)))
    relgap = N * mu / max(1.0, abs(tau))
    if mu_t <= 0 and relgap < 1e-2 and dinf < 1e-2:
        mu_t = 2.0 ** np.round(np.log2(it.get('tol', 2.0 ** -25) * max(1.0, abs(tau))))
    KF = np.concatenate([sr.kron_factors(X1, S1i, V, nx, f)[0], sr.kron_factors(X2, S2i, V, nx, f)[0]], axis=1)
    D, C, _, _ = sr.schur_blocks(KF, p, nx, f)
    cols = sr.rhs_columns_at_iterate(P, tau, alpha, Hb, V, X1, X2, S1, S2, S1i, S2i, nx, f)
    U = cols[:, :, 1:]
    Psi = _sym(X2 @ S2i); Phi2 = _sym(X2 @ Hb @ S2i); PhiH = _sym(X1 @ Hb @ S1i) + Phi2
    btt = np.trace(Psi, axis1=1, axis2=2).sum(); bta = -np.trace(Phi2, axis1=1, axis2=2).sum(); baa = np.sum(Hb * PhiH) + x0 / s0
    K = np.zeros((p * d + 2, p * d + 2))
    K[:p * d, :p * d] = dense_schur(D, C)
    K[:p * d, p * d:] = U.reshape(p * d, 2); K[p * d:, :p * d] = U.reshape(p * d, 2).T
    K[p * d:, p * d:] = [[btt, bta], [bta, baa]]
    X, S, Si, Rd, Li, LXi = (X1, X2), (S1, S2), (S1i, S2i), (Rd1, Rd2), (L1i, L2i), (LX1i, LX2i)

    def direction(sigmu, c, corr0):
        T = [corrector_T(X[r], Rd[r], Si[r], sigmu, None if c is None else c[r], f)[0] for r in (0, 1)]
        q, _ = rhs_partials(T[0], T[1], Hb, f)
        t0 = sigmu / s0 - x0 * rd0 / s0 - corr0
        rhs = np.concatenate([sr.rhs_columns(T[0], T[1], X1, X2, S1i, S2i, Hb, V, nx, f)[0][:, :, 0].ravel(), [q[:, 0].sum() - 1.0, q[:, 1].sum() + t0]])
        sol = np.linalg.solve(K, rhs)
        dtau, dalpha = sol[p * d], sol[p * d + 1]
        dP = np.zeros((p, nx, nx)); v = sol[:p * d].reshape(p, d)
        dP[:, ia, ib] = v; dP[:, ib, ia] = v
        dM, dMb = direction_M(dP, dalpha, Hb, V, nx, f)
        Ldy, Ldyb = linear_parts(dM, dMb, dtau, f)
        dS = [direction_S(Ldy[r], Ldyb[r], Rd[r], f)[0] for r in (0, 1)]
        dX = [direction_X(T[r], X[r], Ldy[r], Ldyb[r], Si[r], f)[0] for r in (0, 1)]
        Wm = np.stack([step_matrix(Li[0], dS[0], f)[0], step_matrix(LXi[0], dX[0], f)[0], step_matrix(Li[1], dS[1], f)[0], step_matrix(LXi[1], dX[1], f)[0]], axis=1)
        eig = np.linalg.eigvalsh(Wm)[..., 0]
        part, _ = partial_sums(dX, dS, X, S, dP, P, dM, dMb, S1, Rd1, dalpha, alpha, f)
        return dict(T=T, dtau=dtau, dalpha=dalpha, dP=dP, dS=dS, dX=dX, Wm=Wm, eig=eig, part=part)

    info = dict(mu=mu, pinf=pinf, dinf=dinf, mu_t=mu_t, rd0=rd0)
    if phase == 0:
        d1 = direction(0.0, None, 0.0)
        sg = sigma_rule(d1['eig'], d1['part'][:, 0], d1['part'][:, 1], d1['part'][:, 2], sxs, x0, s0, mu, mu_t, d1['dalpha'], rd0, N, f)
        c = [corrector_term(d1['dX'][r], d1['dS'][r], Si[r], f)[0] for r in (0, 1)]
        if mutate == 'corrector_sign':
            c = [-c[0], -c[1]]
        sigmu, corr0 = float(sg['sigmu']), float(sg['corr0'])
        info['Wm1'] = d1['Wm']
    else:
        c, sigmu, corr0 = None, mu_t, 0.0
    d2 = direction(sigmu, c, corr0)
    st = step_rule(phase, d2['eig'], d2['part'][:, 5], d2['part'][:, 6], sigmu, corr0, x0, s0, tau, alpha, d2['dtau'], d2['dalpha'], rd0, f)
    ap, ad = float(st['ap']), float(st['ad'])
    nxt = dict(it)
    nxt.update(X1=update(X1, d2['dX'][0], ap, f)[0], X2=update(X2, d2['dX'][1], ap, f)[0], S1=update(S1, d2['dS'][0], ad, f)[0], S2=update(S2, d2['dS'][1], ad, f)[0],
               P=update(P, d2['dP'], ad, f, False)[0], tau=float(st['tau']), alpha=float(st['alpha']), x0=float(st['x0']), s0=float(st['s0']), mu_t=mu_t)
    info.update(sigmu=sigmu, corr0=corr0, ap=ap, ad=ad, rawstep=float(st['rawstep']), stepn=float(st['stepn']), dx0=float(st['dx0']), ds0=float(st['ds0']), Wm2=d2['Wm'],
                **{k: d2[k] for k in ('dtau', 'dalpha', 'dP', 'dS', 'dX')})
    return nxt, info
