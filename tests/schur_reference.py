"""Plain numpy reference of the linear system that one interior-point iteration assembles on the device (k_stage_pre, k_schur, k_stage_rhs, k_gather),
one function per layer, for tests/test_schur_reference_cpu.py and tests/test_gpu_schur_assembly.py.  No device, no oracle import.

Every function takes the INPUTS OF ITS OWN LAYER (on the GPU: as read back from the workspace) and returns (value, bound): the value in `dtype`
(np.longdouble: 64 mantissa bits on x86, 2^11 finer than the fp64 of the kernels) and the absolute-sum bound, the same formula evaluated on the absolute values of
the inputs with every subtraction turned into an addition.  A kernel that forms an entry as m nested fp64 sums / products then errs by at most gamma_m * bound
(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 and (3.13)), whatever its summation order; see gamma().

Shapes: one problem at a time, stage-stacked [p, ...].  n = nx + mb, d = nx (nx + 1) / 2, svec order of np.triu_indices(nx) (row-major upper triangle)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53

# slot order of the Kronecker factors of one LMI (KF_* of csrc/tmpc_common.h); LMI 2 follows LMI 1: 12 slots per stage
KF_XXX, KF_SIXX, KF_KX, KF_KS, KF_FX, KF_FS, KF_PER_LMI = 0, 1, 2, 3, 4, 5, 6


def gamma(m):
    """gamma_m = m eps / (1 - m eps), eps = 2^-53: relative error bound of m nested fp64 roundings"""
    return m * EPS / (1.0 - m * EPS)


def _t(M):
    return np.swapaxes(M, -1, -2)


def _sym(M):
    return (M + _t(M)) / 2


def tri_idx(nx):
    return np.triu_indices(nx)


# ---------------------------------------------------------------------------------------------------------------- inverses
def inverse_residual(S, Si, dtype=LD):
    """S Si - I, stage-stacked"""
    S = np.asarray(S, dtype); Si = np.asarray(Si, dtype)
    return S @ Si - np.eye(S.shape[-1], dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- k_stage_pre: Kronecker factors
def _kron_one(X, Si, V, nx):
    Vt = _t(V)
    return [X[..., :nx, :nx], Si[..., :nx, :nx], V @ X @ Vt, V @ Si @ Vt, X[..., :nx, :] @ Vt, Si[..., :nx, :] @ Vt]


def kron_factors(X, Si, V, nx, dtype=LD):
    """The six nx x nx factors of one LMI block (X, S^-1) [p, n, n] with V = [A B] [p, nx, n], in KF_* order:
    XXX = X[:nx,:nx], SIXX = Si[:nx,:nx], KX = V X V', KS = V Si V', FX = X[:nx,:] V', FS = Si[:nx,:] V'.   -> ([p, 6, nx, nx], bound)"""
    X = np.asarray(X, dtype); Si = np.asarray(Si, dtype); V = np.asarray(V, dtype)
    val = np.stack(_kron_one(X, Si, V, nx), axis=-3)
    bnd = np.stack(_kron_one(np.abs(X), np.abs(Si), np.abs(V), nx), axis=-3)
    return val, bnd


# ---------------------------------------------------------------------------------------------------------------- k_schur: blocks
def _T(L, R, ia, ib):
    """T(L, R)[(ab), (cd)] = <E_ab, L E_cd R'> for the basis E_ab = e_a e_b' + e_b e_a' (a < b), e_a e_a' (a = b), written out:
         L E_cd R' = l_c r_d' + [c != d] l_d r_c'          (l_c, r_c: columns of L, R)   so   M_cd[a, b] = L[a,c] R[b,d] + [c != d] L[a,d] R[b,c]
         <E_ab, M> = M[a, b] + [a != b] M[b, a]
    L, R: [nx, nx] -> [d, d]"""
    a = ia[:, None]; b = ib[:, None]; c = ia[None, :]; e = ib[None, :]
    one = L.dtype.type(1)
    wab = np.where(a != b, one, 0 * one); wcd = np.where(c != e, one, 0 * one)
    m_ab = L[a, c] * R[b, e] + wcd * (L[a, e] * R[b, c])
    m_ba = L[b, c] * R[a, e] + wcd * (L[b, e] * R[a, c])
    return m_ab + wab * m_ba


def schur_blocks(KF, p, nx, dtype=LD):
    """KF [p, 12, nx, nx] -> the diagonal blocks D_k = sum_lmi T(XXX_k, SIXX_k) + T(KX_{k-1}, KS_{k-1}) (stage index mod p) and the coupling blocks
    C_k = T[P_k, P_{k+1}] = -sum_lmi T(FX_k, FS_k), each [p, d, d], and their bounds: (D, C, Dbound, Cbound).  An entry of D is 16 products, of C 8."""
    KF = np.asarray(KF, dtype).reshape(p, 12, nx, nx)
    ia, ib = tri_idx(nx)
    d = len(ia)
    out = []
    for F, sgn in ((KF, -1), (np.abs(KF), 1)):
        D = np.zeros((p, d, d), F.dtype); C = np.zeros((p, d, d), F.dtype)
        for k in range(p):
            km = (k - 1) % p
            for lmi in range(2):
                o = lmi * KF_PER_LMI
                D[k] += _T(F[k, o + KF_XXX], F[k, o + KF_SIXX], ia, ib)
                D[k] += _T(F[km, o + KF_KX], F[km, o + KF_KS], ia, ib)
                C[k] += sgn * _T(F[k, o + KF_FX], F[k, o + KF_FS], ia, ib)
        out.append((D, C))
    return out[0][0], out[0][1], out[1][0], out[1][1]


# ---------------------------------------------------------------------------------------------------------------- k_stage_pre / k_stage_rhs: residuals, T_r
def _calH(V, P, nx, sgn):
    """V' P_{k+1} V - E' P_k E (sgn = -1), stage-stacked; sgn = +1: the bound"""
    out = _t(V) @ np.roll(P, -1, axis=0) @ V
    out[..., :nx, :nx] += sgn * P
    return out


def dual_residuals(P, tau, alpha, Hb, V, S1, S2, nx, dtype=LD):
    """M = alpha Hb + V' P_{k+1} V - E' P_k E;  Rd1 = (M - I) - S1,  Rd2 = (tau I - M) - S2.   -> (Rd1, Rd2, bound1, bound2)"""
    P, Hb, V, S1, S2 = (np.asarray(a, dtype) for a in (P, Hb, V, S1, S2))
    tau = dtype(tau); alpha = dtype(alpha)
    I = np.eye(Hb.shape[-1], dtype=dtype)
    M = alpha * Hb + _calH(V, P, nx, -1)
    Ma = abs(alpha) * np.abs(Hb) + _calH(np.abs(V), np.abs(P), nx, 1)
    return (M - I) - S1, (tau * I - M) - S2, Ma + I + np.abs(S1), abs(tau) * I + Ma + np.abs(S2)


def predictor_T(X, Rd, Si, dtype=LD):
    """T_r = -sym(X_r Rd_r S_r^-1): the predictor (sigma mu = 0, no corrector term).   -> (T, bound)"""
    X, Rd, Si = (np.asarray(a, dtype) for a in (X, Rd, Si))
    return -_sym(X @ Rd @ Si), _sym(np.abs(X) @ np.abs(Rd) @ np.abs(Si))


# ---------------------------------------------------------------------------------------------------------------- k_stage_pre / k_stage_rhs / k_gather: columns
def _svec_grad(G, ia, ib):
    """<E_ab, G> for symmetric G [.., nx, nx]"""
    return G[..., ia, ib] * np.where(ia == ib, 1, 2).astype(G.dtype)


def _calH_adj(V, G, nx, sgn):
    """(calH* G)_j = V_{j-1} G_{j-1} V_{j-1}' - E G_j E' (sgn = -1); sgn = +1: the bound"""
    return np.roll(V @ G @ _t(V), 1, axis=0) + sgn * G[..., :nx, :nx]


def rhs_columns(T1, T2, X1, X2, S1i, S2i, Hb, V, nx, dtype=LD):
    """The three pass-1 columns of the Schur system [p, d, 3]: the predictor right-hand side svec_grad(calH*(T1 - T2)), and the border columns
    u_tau = svec_grad(-calH*(Psi)), Psi = sym(X2 S2^-1), and u_alpha = svec_grad(calH*(PhiH)), PhiH = sym(X1 Hb S1^-1) + sym(X2 Hb S2^-1).   -> (cols, bound)"""
    T1, T2, X1, X2, S1i, S2i, Hb, V = (np.asarray(a, dtype) for a in (T1, T2, X1, X2, S1i, S2i, Hb, V))
    ia, ib = tri_idx(nx)
    out = []
    for sgn, f in ((-1, lambda a: a), (1, np.abs)):
        G = f(T1) + sgn * f(T2)
        Psi = _sym(f(X2) @ f(S2i))
        PhiH = _sym(f(X1) @ f(Hb) @ f(S1i)) + _sym(f(X2) @ f(Hb) @ f(S2i))
        Va = f(V)
        rhs = _svec_grad(_calH_adj(Va, G, nx, sgn), ia, ib)
        ut = _svec_grad(_calH_adj(Va, Psi, nx, sgn), ia, ib)
        ua = _svec_grad(_calH_adj(Va, PhiH, nx, sgn), ia, ib)
        out.append(np.stack([rhs, ut if sgn > 0 else -ut, ua], axis=-1))
    return out[0], out[1]


def rhs_columns_at_iterate(P, tau, alpha, Hb, V, X1, X2, S1, S2, S1i, S2i, nx, dtype=LD):
    """The same columns from the iterate itself: Rd_r from (P, tau, alpha, Hb, S_r), T_r = -sym(X_r Rd_r S_r^-1), then rhs_columns.   -> cols [p, d, 3]"""
    Rd1, Rd2, _, _ = dual_residuals(P, tau, alpha, Hb, V, S1, S2, nx, dtype)
    T1, _ = predictor_T(X1, Rd1, S1i, dtype)
    T2, _ = predictor_T(X2, Rd2, S2i, dtype)
    return rhs_columns(T1, T2, X1, X2, S1i, S2i, Hb, V, nx, dtype)[0]
