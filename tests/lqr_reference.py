"""Plain-numpy statement of the periodic Riccati recursion (test infrastructure of test_lqr_cpu.py / test_gpu_lqr.py; nothing under
tunempc_amd/ imports it).  Stage k of a p-periodic LQ problem, indices mod p, x block of H first:

    E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,  K_k = S^-1 M  (u = -K_k x),  Pi_k = sym(Hb_xx - M' K_k).

A sweep runs k = p-1 ... 0; sweeps repeat until max_k max|dPi_k| / max(1, max|Pi_k|) <= tol.  S goes through np.linalg.solve (LU with
partial pivoting): it is symmetric but in general indefinite."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# the committed vectors that carry A, B, H, Hc, P of plain Step 1 solves
GOLDENS = ['c1_convex_lqr', 'c2_unicycle_shape', 'c3_evaporation_shape', 'mid_n16', 'awe_shape_n15', 'identity_family', 'c5_awe_synthetic_p200_n30']


def load_golden(name):
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: np.ascontiguousarray(d[k], dtype=np.float64) for k in ('A', 'B', 'H', 'Hc', 'P')}


def sweep(A, B, H, Pi):
    """One backward sweep of one problem, in place on Pi [p,nx,nx] -> (K [p,mb,nx], largest relative change, min eig of S over the stages)."""
    p, nx, _ = A.shape
    mb = B.shape[2]
    K = np.zeros((p, mb, nx))
    rel, smin = 0.0, np.inf
    for k in range(p - 1, -1, -1):
        E = np.concatenate([A[k], B[k]], axis=1)
        Hb = H[k] + E.T @ Pi[(k + 1) % p] @ E
        S, M = Hb[nx:, nx:], Hb[nx:, :nx]
        if np.isfinite(S).all():
            smin = min(smin, np.linalg.eigvalsh((S + S.T) / 2).min())
        K[k] = np.linalg.solve(S, M)
        G = Hb[:nx, :nx] - M.T @ K[k]
        new = (G + G.T) / 2
        r = np.abs(new - Pi[k]).max() / max(1.0, np.abs(new).max())
        rel = max(rel, r) if np.isfinite(r) else np.inf
        Pi[k] = new
    return K, rel, smin


def monodromy(A, B, K):
    nx = A.shape[1]
    Phi = np.eye(nx)
    for k in range(A.shape[0]):
        Phi = (A[k] - B[k] @ K[k]) @ Phi
    return Phi


def periodic_lqr(A, B, H, Pi0=None, tol=1e-13, max_sweeps=5000):
    """One problem: A [p,nx,nx], B [p,nx,mb], H [p,n,n] -> dict K, Pi, Phi, rho, sweeps, rel, converged, smin (smallest eigenvalue of S met in
    any sweep)."""
    Pi = np.zeros_like(A) if Pi0 is None else np.array(Pi0, dtype=np.float64)
    smin_all, K, rel, sweeps, conv = np.inf, None, np.inf, 0, False
    with np.errstate(all='ignore'):
        for s in range(max_sweeps):
            K, rel, smin = sweep(A, B, H, Pi)
            sweeps = s + 1
            smin_all = min(smin_all, smin)
            if not np.isfinite(rel):
                break
            if rel <= tol:
                conv = True
                break
    Phi = monodromy(A, B, K)
    rho = np.max(np.abs(np.linalg.eigvals(Phi))) if np.isfinite(Phi).all() else np.nan
    return dict(K=K, Pi=Pi, Phi=Phi, rho=rho, sweeps=sweeps, rel=rel, converged=conv, smin=smin_all)


def periodic_lqr_batch(A, B, H, Pi0=None, tol=1e-13, max_sweeps=5000):
    """A [nb,p,nx,nx], ... -> list of per-problem dicts."""
    return [periodic_lqr(A[b], B[b], H[b], None if Pi0 is None else Pi0[b], tol, max_sweeps) for b in range(A.shape[0])]
