"""Plain numpy reference of the stage-local multiplier rows of an interior-point iteration (tunempc_amd/csrc/tmpc_phi.h: k_phi_pre, k_aug_fill, k_phi_rhs,
k_aug_gather, k_phi_dir, k_phi_steps, k_phi_update), one function per layer, for tests/test_phi_reference_cpu.py and tests/test_gpu_phi_kernels.py.  No device, no
oracle import.  Conventions of tests/schur_reference.py and tests/step_reference.py: every function takes the INPUTS OF ITS OWN LAYER and returns (value, bound), the
value in `dtype` (np.longdouble), the bound the same formula on absolute values with every subtraction turned into an addition.

The model (header comment of tmpc_phi.h; the oracle's rules in oracle/convexify_oracle.py: sdp_step1 with G=, C=, rho=):
  M_k = alpha Hb_k + calH_k(P) + sum_i phi_i g_i g_i', phi_i >= 0 with slack phi_i itself and dual z_i; each norm term an epigraph variable t with the arrow block
  S = arrow(t, v, w) = [[t, w v'], [w v, t I]] >> 0 over the multipliers v under that norm, w = rho sbeta / s, primal X; cost 1 on t.
  The constraint operator, per stage-local variable y, into the cones (LMI 1: S_1 = M - I, LMI 2: S_2 = tau I - M, the linear cone, the arrow blocks):
     A(phi_i) = (+g_i g_i', -g_i g_i', e_i, E_q),  E_q = w (e_0 e_{q+1}' + e_{q+1} e_0') in the arrow block that holds row i as its q-th      A(t) = (0, 0, 0, I)
  HKM Schur entries T[y, y'] = sum_cones <A(y), sym(X A(y') S^-1)>, with x = z, s = phi in the linear cone:
     rows      w_ri = X_r g_i, u_ri = S_r^-1 g_i;  T[phi_i, phi_j] = sum_r (g_i' X_r g_j)(g_i' S_r^-1 g_j) + [i = j] z_i / phi_i + arrow part,
               stored as the Gram form 1/2 (GXG_r[i,j] GSG_r[j,i] + GXG_r[j,i] GSG_r[i,j]), GXG_r[i,j] = g_i . w_rj, GSG_r[i,j] = g_i . u_rj
     border    c_tau_i = T[phi_i, tau] = -(w_2i . u_2i)      c_alpha_i = T[phi_i, alpha] = sum_r w_ri' Hb u_ri
     coupling  a_i = T[phi_i, P_k] = -svec(W_i[:nx, :nx]),  b_i = T[phi_i, P_k+1] = svec(V W_i V'),  W_i = sum_r sym(w_ri u_ri'),  svec = <E_ab, .> (weight 2 off the diagonal)
     arrow     T[phi_a, phi_q] += <E_a, sym(X E_q S^-1)>     T[phi_q, t] = <E_q, sym(X S^-1)>     T[t, t] = tr(X S^-1)
  residuals    r_phi_i = -g_i' (X_1 - X_2) g_i - z_i - 2 w X[0, q+1]     r_t = 1 - tr X
  right-hand   r_loc_i = g_i' (T_1 - T_2) g_i + sig / phi_i - corrp_i + 2 w (sig S^-1 - corr)[0, q+1]     r_loc_t = tr(sig S^-1 - corr) - 1
  sides        (pass 1: sig = 0, no corr; pass 2 main phase: sig = sigma mu, corr of pass 1; centering: sig = mu_t, no corr)
  directions   dy_loc = z_tail - TU_tail (dtau, dalpha)';  dz = sig / phi - z - z dphi / phi - corrp;  corrp = dz dphi / phi (pass 1)
               dS = arrow(dt, dphi, w);  dX = sig S^-1 - X - sym(X dS S^-1) - corr;  acor = sym(dX dS S^-1) (pass 1)
  steps        dual: min(dphi_i / phi_i, min eig L_S^-1 dS L_S^-T, 0); primal: min(dz_i / z_i, min eig L_X^-1 dX L_X^-T, 0); sums <dX,S>, <X,dS>, <dX,dS> with the linear cone
  update       phi += ad dphi, t += ad dt;  z += ap dz, X <- sym(X + ap dX)

Shapes: one stage at a time; X, Si [2, n, n] (LMI 1, LMI 2); G [m, n] the rows present; arrow blocks as (a0, m) over the rows, their matrices (m + 1) x (m + 1)."""
import numpy as np

import schur_reference as sr

LD = sr.LD
_t, _sym = sr._t, sr._sym


def _a(dtype, *arrs):
    return [np.asarray(x, dtype) for x in arrs]


def svec(M, nx):
    """<E_ab, M> over the row-major upper triangle of the leading nx x nx part of symmetric M [.., nx, nx]"""
    ia, ib = sr.tri_idx(nx)
    return M[..., ia, ib] * np.where(ia == ib, 1, 2).astype(M.dtype)


# ---------------------------------------------------------------------------------------------------------------- k_phi_pre: rows
def row_vectors(X, Si, G, dtype=LD):
    """w_ri = X_r g_i, u_ri = S_r^-1 g_i.   -> (w, u [2, m, n], wbound, ubound)"""
    X, Si, G = _a(dtype, X, Si, G)
    f = lambda M, g: np.einsum('rab,ib->ria', M, g)
    return f(X, G), f(Si, G), f(np.abs(X), np.abs(G)), f(np.abs(Si), np.abs(G))


def row_images(V, w, u, dtype=LD):
    """V w_ri, V u_ri.   -> (Vw, Vu [2, m, nx], bounds)"""
    V, w, u = _a(dtype, V, w, u)
    f = lambda V_, x: np.einsum('xa,ria->rix', V_, x)
    return f(V, w), f(V, u), f(np.abs(V), np.abs(w)), f(np.abs(V), np.abs(u))


def border_entries(w, u, Hb, dtype=LD):
    """c_tau_i = -(w_2i . u_2i), c_alpha_i = sum_r w_ri' Hb u_ri.   -> (c_tau, c_alpha [m], bounds)"""
    w, u, Hb = _a(dtype, w, u, Hb)
    ct = -np.sum(w[1] * u[1], axis=-1); ctb = np.sum(np.abs(w[1] * u[1]), axis=-1)
    ca = np.einsum('ria,ab,rib->i', w, Hb, u); cab = np.einsum('ria,ab,rib->i', np.abs(w), np.abs(Hb), np.abs(u))
    return ct, ca, ctb, cab


def gram_products(G, w, u, dtype=LD):
    """GXG_r[i, j] = g_i . w_rj, GSG_r[i, j] = g_i . u_rj.   -> (GXG, GSG [2, m, m], bounds)"""
    G, w, u = _a(dtype, G, w, u)
    f = lambda g, x: np.einsum('ia,rja->rij', g, x)
    return f(G, w), f(G, u), f(np.abs(G), np.abs(w)), f(np.abs(G), np.abs(u))


def rows_block(GXG, GSG, phi, z, dtype=LD):
    """T[phi_i, phi_j] of the two LMIs and the linear cone from the Gram products.   -> (T [m, m], bound)"""
    GXG, GSG, phi, z = _a(dtype, GXG, GSG, phi, z)
    half = dtype(1) / 2
    f = lambda A, B: half * np.sum(A * _t(B) + _t(A) * B, axis=0)
    return f(GXG, GSG) + np.diag(z / phi), f(np.abs(GXG), np.abs(GSG)) + np.diag(np.abs(z / phi))


def rows_residual(GXG, z, dtype=LD):
    """-(g_i' X_1 g_i - g_i' X_2 g_i) - z_i from the diagonals of the Gram products.   -> (r [m], bound)"""
    GXG, z = _a(dtype, GXG, z)
    d0, d1 = np.diagonal(GXG[0]), np.diagonal(GXG[1])
    return -(d0 - d1) - z, np.abs(d0) + np.abs(d1) + np.abs(z)


# ---------------------------------------------------------------------------------------------------------------- k_phi_pre: arrow blocks
def arrow(t, v, wr, dtype=LD):
    """[[t, w v'], [w v, t I]]"""
    v = np.asarray(v, dtype)
    m = len(v)
    S = dtype(t) * np.eye(m + 1, dtype=dtype)
    S[0, 1:] = dtype(wr) * v; S[1:, 0] = dtype(wr) * v
    return S


def inverse(S, dtype=LD):
    """S^-1 in `dtype`: the fp64 inverse refined by two Newton-Schulz steps Y <- Y (2 I - S Y) (numpy has no extended-precision LAPACK)"""
    S = np.asarray(S, dtype)
    Y = np.asarray(np.linalg.inv(np.asarray(S, np.float64)), dtype)
    I2 = 2 * np.eye(S.shape[-1], dtype=dtype)
    for _ in range(2):
        Y = Y @ (I2 - S @ Y)
    return Y


def _E(q, m, wr, dtype):
    E = np.zeros((m + 1, m + 1), dtype)
    E[0, q + 1] = E[q + 1, 0] = dtype(wr)
    return E


def arrow_schur(X, Si, wr, dtype=LD):
    """the entries of one arrow block (X, S^-1 its (m+1) x (m+1) matrices): Tqq[a, q] = <E_a, sym(X E_q S^-1)>, Tqt[q] = <E_q, sym(X S^-1)>, Ttt = tr(X S^-1).
    -> (Tqq [m, m], Tqt [m], Ttt, bounds of the three)"""
    X, Si = _a(dtype, X, Si)
    m = X.shape[0] - 1
    out = []
    for sgn_abs in (False, True):
        Xa, Sa = (np.abs(X), np.abs(Si)) if sgn_abs else (X, Si)
        w_ = abs(dtype(wr)) if sgn_abs else dtype(wr)
        Tqq = np.zeros((m, m), dtype)
        for q in range(m):
            F = _sym(Xa @ _E(q, m, w_, dtype) @ Sa)
            Tqq[:, q] = 2 * w_ * F[0, 1:]                      # <E_a, F> = w (F[0, a+1] + F[a+1, 0])
        Pe = _sym(Xa @ Sa)
        out += [Tqq, 2 * w_ * Pe[0, 1:], np.trace(Pe)]
    return tuple(out)


def arrow_residual(X, wr, dtype=LD):
    """what the arrow block adds to the stationarity residual of its rows, and the residual of its epigraph variable.   -> (rq [m], rt, bounds)"""
    X = np.asarray(X, dtype)
    w_ = dtype(wr)
    return -2 * w_ * X[0, 1:], 1 - np.trace(X), 2 * abs(w_) * np.abs(X[0, 1:]), 1 + np.trace(np.abs(X))


def complementarity(phi, z, arrows=(), dtype=LD):
    """what k_phi_pre adds to Q_XS: phi . z + sum <X, S> over the arrow blocks [(X, S)].   -> (value, bound)"""
    phi, z = _a(dtype, phi, z)
    v = np.sum(phi * z); b = np.sum(np.abs(phi * z))
    for X, S in arrows:
        X, S = _a(dtype, X, S)
        v = v + np.sum(X * S); b = b + np.sum(np.abs(X * S))
    return v, b


# ---------------------------------------------------------------------------------------------------------------- k_aug_fill: coupling to P
def coupling_rows(w, u, Vw, Vu, nx, dtype=LD):
    """a_i = -svec(W_i[:nx, :nx]) (P_k), b_i = svec(V W_i V') (P_k+1) with W_i = sum_r sym(w_ri u_ri').   -> (a, b [m, d], bounds)"""
    w, u, Vw, Vu = _a(dtype, w, u, Vw, Vu)
    f = lambda x, y: svec(np.sum(_sym(x[..., :, None] * y[..., None, :]), axis=0), nx)
    a = -f(w[..., :nx], u[..., :nx]); b = f(Vw, Vu)
    return a, b, f(np.abs(w[..., :nx]), np.abs(u[..., :nx])), f(np.abs(Vw), np.abs(Vu))


# ---------------------------------------------------------------------------------------------------------------- k_phi_rhs: right-hand sides
def rhs_rows(T1, T2, G, phi, sig, corrp=None, dtype=LD):
    """g_i' (T_1 - T_2) g_i + sig / phi_i - corrp_i.   -> (r [m], bound)"""
    T1, T2, G, phi = _a(dtype, T1, T2, G, phi)
    sg = dtype(sig)
    r = np.einsum('ia,ab,ib->i', G, T1 - T2, G) + sg / phi
    b = np.einsum('ia,ab,ib->i', np.abs(G), np.abs(T1) + np.abs(T2), np.abs(G)) + np.abs(sg / phi)
    if corrp is not None:
        corrp = np.asarray(corrp, dtype)
        r = r - corrp; b = b + np.abs(corrp)
    return r, b


def arrow_rhs(Si, sig, wr, cor=None, dtype=LD):
    """T_e = sig S^-1 - corr: the rows gain 2 w T_e[0, q+1], the epigraph variable has tr T_e - 1.   -> (rq [m], rt, bounds)"""
    Si = np.asarray(Si, dtype)
    sg, w_ = dtype(sig), dtype(wr)
    Te = sg * Si; Tb = np.abs(sg * Si)
    if cor is not None:
        cor = np.asarray(cor, dtype)
        Te = Te - cor; Tb = Tb + np.abs(cor)
    return 2 * w_ * Te[0, 1:], np.trace(Te) - 1, 2 * abs(w_) * Tb[0, 1:], np.trace(Tb) + 1


# ---------------------------------------------------------------------------------------------------------------- k_phi_dir: directions
def local_direction(Zt, TUt, dtau, dalpha, dtype=LD):
    """dy_loc = z_tail - TU_tail (dtau, dalpha)' from the tail of the block solution.   -> (dy [nz], bound)"""
    Zt, TUt = _a(dtype, Zt, TUt)
    dt, da = dtype(dtau), dtype(dalpha)
    return Zt - TUt[:, 0] * dt - TUt[:, 1] * da, np.abs(Zt) + np.abs(TUt[:, 0] * dt) + np.abs(TUt[:, 1] * da)


def dual_direction(phi, z, dphi, sig, corrp=None, dtype=LD):
    """dz = sig / phi - z - z dphi / phi - corrp.   -> (dz [m], bound)"""
    phi, z, dphi = _a(dtype, phi, z, dphi)
    sg = dtype(sig)
    v = sg / phi - z - z * dphi / phi
    b = np.abs(sg / phi) + np.abs(z) + np.abs(z * dphi / phi)
    if corrp is not None:
        corrp = np.asarray(corrp, dtype)
        v = v - corrp; b = b + np.abs(corrp)
    return v, b


def mehrotra_rows(dz, dphi, phi, dtype=LD):
    """corrp = dz dphi / phi.   -> (corrp [m], bound)"""
    dz, dphi, phi = _a(dtype, dz, dphi, phi)
    v = dz * dphi / phi
    return v, np.abs(v)


def arrow_dX(X, Si, dS, sig, cor=None, dtype=LD):
    """dX = sig S^-1 - X - sym(X dS S^-1) - corr.   -> (dX, bound)"""
    X, Si, dS = _a(dtype, X, Si, dS)
    sg = dtype(sig)
    v = sg * Si - X - _sym(X @ dS @ Si)
    b = np.abs(sg * Si) + np.abs(X) + _sym(np.abs(X) @ np.abs(dS) @ np.abs(Si))
    if cor is not None:
        cor = np.asarray(cor, dtype)
        v = v - cor; b = b + np.abs(cor)
    return v, b


def arrow_corrector(dX, dS, Si, dtype=LD):
    """acor = sym(dX dS S^-1).   -> (acor, bound)"""
    dX, dS, Si = _a(dtype, dX, dS, Si)
    return _sym(dX @ dS @ Si), _sym(np.abs(dX) @ np.abs(dS) @ np.abs(Si))


def arrow_sums(dX, S, X, dS, dtype=LD):
    """<dX, S>, <X, dS>, <dX, dS>.   -> ([3], bound)"""
    dX, S, X, dS = _a(dtype, dX, S, X, dS)
    f = lambda a, b: np.sum(a * b)
    return (np.array([f(dX, S), f(X, dS), f(dX, dS)], dtype),
            np.array([f(np.abs(dX), np.abs(S)), f(np.abs(X), np.abs(dS)), f(np.abs(dX), np.abs(dS))], dtype))


def step_matrix(Li, D, dtype=LD):
    """sym(L^-1 D L^-T): its smallest eigenvalue bounds the step.   -> (W, bound)"""
    Li, D = _a(dtype, Li, D)
    return _sym(Li @ D @ _t(Li)), _sym(np.abs(Li) @ np.abs(D) @ _t(np.abs(Li)))


# ---------------------------------------------------------------------------------------------------------------- k_phi_steps
def linear_cone_steps(phi, z, dphi, dz):
    """min_i dphi_i / phi_i (dual) and min_i dz_i / z_i (primal) in fp64: a division is correctly rounded and a minimum exact, so the device value is THIS number.
    -> (ls, lx); +inf without rows"""
    phi, z, dphi, dz = _a(np.float64, phi, z, dphi, dz)
    if len(phi) == 0:
        return np.inf, np.inf
    return float(np.min(dphi / phi)), float(np.min(dz / z))


def linear_cone_sums(phi, z, dphi, dz, dtype=LD):
    """dz . phi, z . dphi, dz . dphi: what the linear cone adds to Q_DXS, Q_XDS, Q_DXDS.   -> ([3], bound)"""
    phi, z, dphi, dz = _a(dtype, phi, z, dphi, dz)
    v = np.array([np.sum(dz * phi), np.sum(z * dphi), np.sum(dz * dphi)], dtype)
    b = np.array([np.sum(np.abs(dz * phi)), np.sum(np.abs(z * dphi)), np.sum(np.abs(dz * dphi))], dtype)
    return v, b


# ---------------------------------------------------------------------------------------------------------------- k_phi_update
def update(x, dx, a, symmetric=False, dtype=LD):
    """x + a dx (symmetrised for the arrow X).   -> (value, bound)"""
    x, dx = _a(dtype, x, dx)
    v = x + dtype(a) * dx; b = np.abs(x) + np.abs(dtype(a) * dx)
    return (_sym(v), _sym(b)) if symmetric else (v, b)


# ---------------------------------------------------------------------------------------------------------------- one stage, layer by layer
def stage_system(X, Si, V, Hb, G, phi, z, nx, arrows=(), wr=0.0, dtype=LD, mut=None):
    """Everything k_phi_pre and k_aug_fill produce for one stage from the iterate, each layer from the layer before in `dtype`: dict of T_loc,loc [nz, nz]
    (rows, then one epigraph variable per arrow block), c_tau, c_alpha [nz] (zero at the epigraph variables), a, b [m, d], res [nz].
    arrows: [(a0, m, t, Xa)]; S is rebuilt from (t, phi).  mut: one numerical mutation of profiles/phi_kernel_mutations.txt applied to the reference."""
    m = len(G)
    nz = m + len(arrows)
    w, u, _, _ = row_vectors(X, Si, G, dtype)
    Vw, Vu, _, _ = row_images(V, w, u, dtype)
    ct, ca, _, _ = border_entries(w, u, Hb, dtype)
    if mut == 'c_tau_sign':
        ct = -ct
    GXG, GSG, _, _ = gram_products(G, w, u, dtype)
    if mut == 'gsg_other_cone':
        GSG = GSG[::-1]
    Trr, _ = rows_block(GXG, GSG, phi, z, dtype)
    res, _ = rows_residual(GXG, z, dtype)
    a, b, _, _ = coupling_rows(w, u, Vw, Vu, nx, dtype)
    if mut == 'a_b_swapped':
        a, b = b, a
    T = np.zeros((nz, nz), dtype); T[:m, :m] = Trr
    res = np.concatenate([res, np.zeros(len(arrows), dtype)])
    for e, (a0, am, t, Xa) in enumerate(arrows):
        S = arrow(t, np.asarray(phi, dtype)[a0:a0 + am], wr, dtype)
        Sai = inverse(S, dtype)
        Tqq, Tqt, Ttt = arrow_schur(Xa, Sai, wr, dtype)[:3]
        T[a0:a0 + am, a0:a0 + am] += Tqq
        T[a0:a0 + am, m + e] = Tqt; T[m + e, a0:a0 + am] = Tqt; T[m + e, m + e] = Ttt
        rq, rt = arrow_residual(Xa, wr, dtype)[:2]
        if mut == 'arrow_residual_factor':
            rq = rq / 2
        res[a0:a0 + am] += rq; res[m + e] = rt
    pad = np.zeros(len(arrows), dtype)
    return dict(T=T, c_tau=np.concatenate([ct, pad]), c_alpha=np.concatenate([ca, pad]), a=a, b=b, res=res, w=w, u=u, Vw=Vw, Vu=Vu, GXG=GXG, GSG=GSG)
