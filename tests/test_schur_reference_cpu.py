"""tests/schur_reference.py against the CPU oracle, against brute force, and against its own rounding bounds (no device).

The GPU test (tests/test_gpu_schur_assembly.py) compares every assembly kernel with this reference inside a derived rounding bound 4 gamma_m * (absolute-sum
bound).  Here: the reference computes what the oracle computes; the same formulas in plain fp64 numpy stay inside those bounds (so a correct kernel can);
and every problem of the GPU test is still in the main phase, by the oracle's own trace, at the iteration the GPU test stops at."""
import numpy as np
import pytest

import convexify_oracle as co
import schur_reference as sr
from schur_assembly_cases import CASES, make_problem, solved_members

LD = np.longdouble


def test_longdouble_is_wider_than_fp64():
    # the reference must resolve the bounds it is compared inside: 4 gamma_m >= 2^-50
    assert np.finfo(LD).eps <= 2.0 ** -60


def _spd(rng, p, n, cond):
    out = np.empty((p, n, n))
    for k in range(p):
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = 10.0 ** rng.uniform(-np.log10(cond) / 2, np.log10(cond) / 2, n)
        lam[0] = cond ** -0.5; lam[-1] = cond ** 0.5
        out[k] = co.symmetrize((Q * lam) @ Q.T)
    return out


def _iterate(seed, p, nx, mb, cond=10.0):
    """synthetic 'live' iterate: SPD X1 != X2, S1 != S2, V = [A B], symmetric Hb and P"""
    rng = np.random.default_rng(seed)
    n = nx + mb
    X1, X2, S1, S2 = (_spd(rng, p, n, c) for c in (10.0, 30.0, cond, cond))
    V = rng.standard_normal((p, nx, n)) / np.sqrt(nx)
    Hb = co.symmetrize(rng.standard_normal((p, n, n)))
    P = co.symmetrize(rng.standard_normal((p, nx, nx)))
    return dict(X1=X1, X2=X2, S1=S1, S2=S2, V=V, Hb=Hb, P=P, A=V[:, :, :nx].copy(), B=V[:, :, nx:].copy(), tau=1.7, alpha=0.3)


def _chol_inverse_fp64(S):
    """S^-1 the way the stage kernels form it: S = L L', L^-1, sym(L^-T L^-1), all fp64"""
    L = np.linalg.cholesky(S)
    Li = np.stack([np.linalg.solve(L[k], np.eye(S.shape[-1])) for k in range(S.shape[0])])
    return co.symmetrize(np.swapaxes(Li, 1, 2) @ Li)


def _kf12(it, Si1, Si2, nx, dtype=LD):
    f1, b1 = sr.kron_factors(it['X1'], Si1, it['V'], nx, dtype)
    f2, b2 = sr.kron_factors(it['X2'], Si2, it['V'], nx, dtype)
    return np.concatenate([f1, f2], axis=1), np.concatenate([b1, b2], axis=1)


def _rel(got, ref):
    return float(np.abs(np.asarray(got, LD) - np.asarray(ref, LD)).max() / np.abs(np.asarray(ref, LD)).max())


@pytest.mark.parametrize('nx', [1, 2, 5])
@pytest.mark.parametrize('p', [1, 2, 3])
def test_blocks_match_oracle_assembly(p, nx):
    mb = 2
    it = _iterate(100 * p + nx, p, nx, mb)
    S1i = np.linalg.inv(it['S1']); S2i = np.linalg.inv(it['S2'])
    ia, ib = co._tri_idx(nx)
    d = len(ia)
    Vt = np.swapaxes(it['V'], 1, 2)
    # the oracle's fp64 assembly, convexify_oracle.py: _blocks64 inside sdp_step1
    D_ = np.zeros((p, d, d)); C_ = np.zeros((p, d, d))
    for X, Si in ((it['X1'], S1i), (it['X2'], S2i)):
        Kx = it['V'] @ X @ Vt; Ks = it['V'] @ Si @ Vt
        Fx = X[:, :nx, :] @ Vt; Fs = Si[:, :nx, :] @ Vt
        D_ += co._hkm_block(X[:, :nx, :nx], Si[:, :nx, :nx], ia, ib)
        D_ += np.roll(co._hkm_block(Kx, Ks, ia, ib), 1, axis=0)
        C_ -= co._hkm_block(Fx, Fs, ia, ib)
    KF, _ = _kf12(it, S1i, S2i, nx)
    D, C, Db, Cb = sr.schur_blocks(KF, p, nx)
    assert D.shape == (p, d, d) and C.shape == (p, d, d)
    assert _rel(D, D_) <= 1e-13 and _rel(C, C_) <= 1e-13, (_rel(D, D_), _rel(C, C_))
    # ... and its double-double assembly (tight mode)
    Dd, Cd = co._assemble_dd(it['X1'], S1i, it['X2'], S2i, it['V'], nx, ia, ib)
    Dd = np.asarray(Dd.hi, LD) + np.asarray(Dd.lo, LD); Cd = np.asarray(Cd.hi, LD) + np.asarray(Cd.lo, LD)
    assert _rel(D, Dd) <= 1e-13 and _rel(C, Cd) <= 1e-13, (_rel(D, Dd), _rel(C, Cd))
    # the bounds dominate the values, and D is as symmetric as its factors (np.linalg.inv returns S^-1 symmetric to fp64 rounding only)
    assert np.all(Db >= np.abs(D)) and np.all(Cb >= np.abs(C))
    assert _rel(D, np.swapaxes(D, 1, 2)) <= 1e-14


def test_T_matches_brute_force_kronecker():
    nx = 3
    rng = np.random.default_rng(7)
    L = rng.standard_normal((nx, nx)); R = rng.standard_normal((nx, nx))       # (not symmetric: the F factors are not)
    ia, ib = sr.tri_idx(nx)
    d = len(ia)
    Dn = np.zeros((nx * nx, d))                    # vec(E_ab) = Dn[:, (ab)], row-major vec
    for e, (a, b) in enumerate(zip(ia, ib)):
        Dn[a * nx + b, e] = 1.0; Dn[b * nx + a, e] = 1.0
    brute = Dn.T @ np.kron(L, R) @ Dn
    assert _rel(sr._T(L.astype(LD), R.astype(LD), ia, ib), brute) <= 1e-15
    # entry by entry from the definition <E_ab, L E_cd R'>
    for e in range(d):
        E_cd = Dn[:, e].reshape(nx, nx)
        M = L @ E_cd @ R.T
        for f in range(d):
            assert abs(float(sr._T(L.astype(LD), R.astype(LD), ia, ib)[f, e]) - np.sum(Dn[:, f].reshape(nx, nx) * M)) <= 1e-14


@pytest.mark.parametrize('p,nx,mb', [(1, 2, 1), (2, 3, 1), (3, 5, 2)])
def test_rhs_columns_match_oracle_at_initial_point(p, nx, mb):
    A, B, H, _, _ = co.gen_problem(900 + p, p, nx, mb)
    n = nx + mb
    s, sbeta = co.auto_scaling(H); Hb = s * H
    I = np.eye(n)
    tau, alpha, x0 = 2.0, 1.0 / sbeta, 1.0 / (p * n)
    P = np.zeros((p, nx, nx))
    S1 = np.broadcast_to(I, (p, n, n)).copy(); S2 = tau * I - alpha * Hb
    X1 = np.broadcast_to(x0 * I, (p, n, n)).copy(); X2 = X1.copy()
    S1i = np.linalg.inv(S1); S2i = np.linalg.inv(S2)
    ia, ib = co._tri_idx(nx)
    # convexify_oracle.py, sdp_step1: the residuals, the border columns and direction(sig_mu = 0)
    M = alpha * Hb + co.calH(A, B, P)
    Rd1 = (M - I) - S1; Rd2 = (tau * I - M) - S2
    Psi = co.symmetrize(X2 @ S2i)
    PhiH = co.symmetrize(X1 @ Hb @ S1i) + co.symmetrize(X2 @ Hb @ S2i)
    u_tau = co._svec_grad(-co.calH_adj(A, B, Psi), ia, ib)
    u_alpha = co._svec_grad(co.calH_adj(A, B, PhiH), ia, ib)
    T1 = -co.symmetrize(X1 @ Rd1 @ S1i); T2 = -co.symmetrize(X2 @ Rd2 @ S2i)
    rhs_P = co._svec_grad(co.calH_adj(A, B, T1 - T2), ia, ib)
    V = np.concatenate([A, B], axis=2)
    cols = sr.rhs_columns_at_iterate(P, tau, alpha, Hb, V, X1, X2, S1, S2, S1i, S2i, nx)
    for j, ref in enumerate((rhs_P, u_tau, u_alpha)):
        assert _rel(cols[:, :, j], ref) <= 1e-13, (j, _rel(cols[:, :, j], ref))
    r1, r2, _, _ = sr.dual_residuals(P, tau, alpha, Hb, V, S1, S2, nx)
    # (Rd2 is a rounding residue at the starting point, S2 = fl(tau I - alpha Hb): both residuals on the scale of Rd1)
    assert _rel(np.stack([r1, r2]), np.stack([Rd1, Rd2])) <= 1e-13


@pytest.mark.parametrize('cond', [1e1, 1e4, 1e8])
@pytest.mark.parametrize('p,nx,mb', [(1, 2, 1), (2, 3, 1), (3, 5, 2), (2, 10, 3)])
def test_fp64_evaluation_stays_inside_the_bounds(p, nx, mb, cond):
    """Every inequality of the GPU test, with the same formulas in plain fp64 numpy in the place of the kernels: the bounds leave room for a correct fp64 evaluation,
    at cond(S) up to 1e8 and X1 != X2."""
    it = _iterate(int(np.log10(cond)) * 1000 + 10 * p + nx, p, nx, mb, cond)
    n = nx + mb
    f64 = np.float64
    # inverses: ||S Si - I||_max <= 4 gamma_{3n} cond_2(S)
    Si = {}
    for r in (1, 2):
        S = it[f'S{r}']
        Si[r] = _chol_inverse_fp64(S)
        res = np.abs(sr.inverse_residual(S, Si[r])).max(axis=(1, 2))
        assert np.all(res <= 4 * sr.gamma(3 * n) * np.linalg.cond(S)), (r, res, np.linalg.cond(S))
    # Kronecker factors from the fp64 inverses: 2n terms
    KF64, _ = _kf12(it, Si[1], Si[2], nx, f64)
    KF, KFb = _kf12(it, Si[1], Si[2], nx)
    assert np.all(np.abs(KF64 - KF) <= 4 * sr.gamma(2 * n) * KFb)
    # blocks from the fp64 factors: 16 / 8 products, gamma_32
    D64, C64, _, _ = sr.schur_blocks(KF64, p, nx, f64)
    D, C, Db, Cb = sr.schur_blocks(KF64, p, nx)
    assert np.all(np.abs(D64 - D) <= 4 * sr.gamma(32) * Db) and np.all(np.abs(C64 - C) <= 4 * sr.gamma(32) * Cb)
    # residuals (2 nx + 5 terms), T_r (3n), columns (4n), each from the fp64 values of the layer before
    a = (it['P'], it['tau'], it['alpha'], it['Hb'], it['V'], it['S1'], it['S2'], nx)
    Rd64 = sr.dual_residuals(*a, f64)
    Rd = sr.dual_residuals(*a)
    T64 = []
    for r in (1, 2):
        assert np.all(np.abs(Rd64[r - 1] - Rd[r - 1]) <= 4 * sr.gamma(2 * nx + 5) * Rd[r + 1])
        t64, _ = sr.predictor_T(it[f'X{r}'], Rd64[r - 1], Si[r], f64)
        t, tb = sr.predictor_T(it[f'X{r}'], Rd64[r - 1], Si[r])
        assert np.all(np.abs(t64 - t) <= 4 * sr.gamma(3 * n) * tb)
        T64.append(t64)
    c64, _ = sr.rhs_columns(T64[0], T64[1], it['X1'], it['X2'], Si[1], Si[2], it['Hb'], it['V'], nx, f64)
    c, cb = sr.rhs_columns(T64[0], T64[1], it['X1'], it['X2'], Si[1], Si[2], it['Hb'], it['V'], nx)
    assert np.all(np.abs(c64 - c) <= 4 * sr.gamma(4 * n) * cb)


@pytest.mark.parametrize('shape', sorted({c[0] for c in CASES}))
def test_gpu_cases_are_in_the_main_phase_at_their_stop_iteration(shape):
    """sdp_step1 reports phase 0 (main) at every iteration up to the largest K of the shape, for every member the solver iterates on; the member
    that leaves at the pre-check is positive definite."""
    nb, p, nx, mb = shape
    kmax = max(k for s, k in CASES if s == shape)
    A, B, H = make_problem(shape)
    solved = solved_members(shape)
    for b in range(nb):
        definite = np.linalg.eigvalsh(co.symmetrize(H[b]))[:, 0].min() > 0
        assert definite == (b not in solved)
        if not definite:
            trace = []
            co.sdp_step1(A[b], B[b], co.symmetrize(H[b]), dict(max_iter=kmax), trace=trace)
            assert len(trace) >= kmax and all(t['phase'] == 0 for t in trace[:kmax]), [(t['it'], t['phase']) for t in trace]
