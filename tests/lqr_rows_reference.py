"""Plain-numpy statement of the periodic Riccati recursion with the rows of G_k / C_k held as equalities (test infrastructure of test_lqr_rows_cpu.py /
test_gpu_lqr_rows.py; nothing under tunempc_amd/ imports it).  Stage k of a p-periodic LQ problem, indices mod p, x block of H first, rows
J_k = [Jx | Ju] (r_k x (nx + mb), r_k <= mb, Ju of full row rank) with J_k [x_k; u_k] = 0:

    E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,  u = -K_k x with Ju K_k = Jx.

Two forms of the stage solve.  The kernel (csrc/tmpc_lqr_rows.h) eliminates on the KKT matrix; the reference of the GPU tests is the OTHER one:

  'nullspace' (default): Ju' = [Y Z] R (complete QR),  K = Y R^-T Jx + Z (Z'SZ)^-1 Z'(M - S Y R^-T Jx),  Pi_k = sym(T' Hb T), T = [I; -K],
                         Lam = R^-1 Y'(M - S K)   (from S K + Ju' Lam = M);
  'kkt':                 [[S, Ju'], [Ju, 0]] [K; Lam] = [M; Jx] by np.linalg.solve,  Pi_k = sym(Hb_xx - [M; Jx]' [K; Lam]).

A stage with r_k = 0 is the stage of lqr_reference.sweep, expression for expression.  A sweep runs k = p-1 ... 0; sweeps repeat until
max_k max|dPi_k| / max(1, max|Pi_k|) <= tol."""
import numpy as np

import lqr_reference as lr


def stage(Hb, Jk, nx, method='nullspace'):
    """One stage solve -> (K [mb,nx], Lam [r,nx], Pi_k before nothing else: symmetrised)."""
    S, M = Hb[nx:, nx:], Hb[nx:, :nx]
    mb = S.shape[0]
    r = 0 if Jk is None else Jk.shape[0]
    if r == 0:
        K = np.linalg.solve(S, M)
        G = Hb[:nx, :nx] - M.T @ K
        return K, np.zeros((0, nx)), (G + G.T) / 2
    Jx, Ju = Jk[:, :nx], Jk[:, nx:]
    if method == 'kkt':
        KKT = np.block([[S, Ju.T], [Ju, np.zeros((r, r))]])
        sol = np.linalg.solve(KKT, np.concatenate([M, Jx], axis=0))
        K, Lam = sol[:mb], sol[mb:]
        G = Hb[:nx, :nx] - np.concatenate([M, Jx], axis=0).T @ sol
        return K, Lam, (G + G.T) / 2
    Q, R = np.linalg.qr(Ju.T, mode='complete')
    Y, Z, R1 = Q[:, :r], Q[:, r:], R[:r]
    Ky = np.linalg.solve(R1.T, Jx)
    K = Y @ Ky
    if r < mb:
        K = K + Z @ np.linalg.solve(Z.T @ S @ Z, Z.T @ (M - S @ K))
    Lam = np.linalg.solve(R1, Y.T @ (M - S @ K))
    T = np.concatenate([np.eye(nx), -K], axis=0)
    G = T.T @ Hb @ T
    return K, Lam, (G + G.T) / 2


def sweep(A, B, H, Pi, J, rows, method='nullspace'):
    """One backward sweep of one problem, in place on Pi [p,nx,nx].  J [p,nr,n], rows [p] (r_k) -> (K [p,mb,nx], Lam [p,nr,nx], largest relative change)."""
    p, nx, _ = A.shape
    mb = B.shape[2]
    nr = 0 if J is None else J.shape[1]
    K = np.zeros((p, mb, nx)); Lam = np.zeros((p, nr, nx))
    rel = 0.0
    for k in range(p - 1, -1, -1):
        E = np.concatenate([A[k], B[k]], axis=1)
        Hb = H[k] + E.T @ Pi[(k + 1) % p] @ E
        rk = int(rows[k]) if nr else 0
        K[k], Lam[k, :rk], new = stage(Hb, J[k, :rk] if rk else None, nx, method)
        r = np.abs(new - Pi[k]).max() / max(1.0, np.abs(new).max())
        rel = max(rel, r) if np.isfinite(r) else np.inf
        Pi[k] = new
    return K, Lam, rel


def periodic_lqr(A, B, H, J=None, rows=None, Pi0=None, tol=1e-13, max_sweeps=5000, method='nullspace'):
    """One problem: A [p,nx,nx], B [p,nx,mb], H [p,n,n], J [p,nr,n], rows [p] (None: all nr rows at every stage) -> dict K, Pi, Phi, Lam, rho, sweeps,
    rel, converged, feas (max_k max|Jx - Ju K_k|)."""
    p, nx = A.shape[0], A.shape[1]
    if J is not None and rows is None:
        rows = np.full(p, J.shape[1])
    Pi = np.zeros_like(A) if Pi0 is None else np.array(Pi0, dtype=np.float64)
    K, Lam, rel, sweeps, conv = None, None, np.inf, 0, False
    with np.errstate(all='ignore'):
        for s in range(max_sweeps):
            K, Lam, rel = sweep(A, B, H, Pi, J, rows, method)
            sweeps = s + 1
            if not np.isfinite(rel):
                break
            if rel <= tol:
                conv = True
                break
    Phi = lr.monodromy(A, B, K)
    rho = np.max(np.abs(np.linalg.eigvals(Phi))) if np.isfinite(Phi).all() else np.nan
    feas = 0.0
    if J is not None:
        for k in range(p):
            rk = int(rows[k])
            if rk:
                feas = max(feas, np.abs(J[k, :rk, :nx] - J[k, :rk, nx:] @ K[k]).max())
    return dict(K=K, Pi=Pi, Phi=Phi, Lam=Lam, rho=rho, sweeps=sweeps, rel=rel, converged=conv, feas=feas)


def periodic_lqr_batch(A, B, H, J=None, rows=None, Pi0=None, tol=1e-13, max_sweeps=5000, method='nullspace'):
    """A [nb,p,nx,nx], ..., J [nb,p,nr,n], rows [nb,p] -> list of per-problem dicts."""
    return [periodic_lqr(A[b], B[b], H[b], None if J is None else J[b], None if rows is None else rows[b], None if Pi0 is None else Pi0[b],
                         tol, max_sweeps, method) for b in range(A.shape[0])]


def gen_rows(seed, nb, p, n, ng, nc):
    """Random rows in the layout of the Step 2 entries: J [nb,p,ng+nc,n] (rows beyond ng + ncnt zero), ncnt [nb,p] int32 in 0 .. nc."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nb, p, ng, n)); C = rng.standard_normal((nb, p, nc, n))
    ncnt = rng.integers(0, nc + 1, size=(nb, p)).astype(np.int32)
    for b in range(nb):
        for k in range(p):
            C[b, k, ncnt[b, k]:] = 0.0
    return np.concatenate([G, C], axis=2), ncnt
