"""Plain-numpy statement of the closed-loop rollout (test infrastructure of test_closed_loop_cpu.py / test_gpu_closed_loop.py; nothing under tunempc_amd/
imports it).  One problem at a time, a loop over the steps:

    U = -K_k X,  Z = [X; U],  l = 1/2 colsum(Z o (H_k Z)),  lc likewise on Hc_k,  rowres = colmax|J_k Z| over the first r_k rows,
    subres = colmax|Hn_k X|,  X <- A_k X + B_k U,   k = (k0 + t) mod p.

The cases are those of lqr_horizon_reference (imported, not edited), each with a seeded random feedback K and initial states X0.  A random K is not a
stabilising one: the trajectories grow, which is what the telescoping identity is to be tested on (it holds for ANY feedback)."""
import numpy as np

import lqr_horizon_reference as lh


def rollout(A, B, K, X0, T, k0=0, H=None, Hc=None, J=None, rows=None, Hn=None):
    """A [p,nx,nx], B [p,nx,mb], K [p,mb,nx], X0 [ns,nx]; H, Hc [p,n,n], J [p,nr,n] with rows [p] (None: all nr), Hn [p,nx,nx], each or None ->
    dict X [ns,T+1,nx], U [ns,T,mb], l, lc, rowres, subres [ns,T] (None without their input), XT [ns,nx], L, Lc [ns]."""
    p, nx = A.shape[0], A.shape[1]
    mb = B.shape[2]
    ns = X0.shape[0]
    X = np.zeros((ns, T + 1, nx)); U = np.zeros((ns, T, mb))
    out = {k: (np.zeros((ns, T)) if have is not None else None) for k, have in (('l', H), ('lc', Hc), ('rowres', J), ('subres', Hn))}
    x = np.array(X0, dtype=np.float64).T                                       # [nx, ns]
    X[:, 0] = x.T
    for t in range(T):
        k = (k0 + t) % p
        u = -(K[k] @ x)
        z = np.concatenate([x, u], axis=0)
        U[:, t] = u.T
        if H is not None:
            out['l'][:, t] = 0.5 * (z * (H[k] @ z)).sum(axis=0)
        if Hc is not None:
            out['lc'][:, t] = 0.5 * (z * (Hc[k] @ z)).sum(axis=0)
        if J is not None:
            rk = J.shape[1] if rows is None else int(rows[k])
            out['rowres'][:, t] = np.abs(J[k, :rk] @ z).max(axis=0) if rk else 0.0
        if Hn is not None:
            out['subres'][:, t] = np.abs(Hn[k] @ x).max(axis=0)
        x = A[k] @ x + B[k] @ u
        X[:, t + 1] = x.T
    out.update(X=X, U=U, XT=X[:, T].copy(), L=None if H is None else out['l'].sum(axis=1), Lc=None if Hc is None else out['lc'].sum(axis=1))
    return out


def monodromy_rollout(A, B, K, Pz0=None):
    """The rollout of the columns of I (or Pz0) over one period from phase 0 -> Phi [nx,nx]."""
    nx = A.shape[1]
    X0 = np.eye(nx) if Pz0 is None else np.asarray(Pz0).T
    return rollout(A, B, K, X0, A.shape[0])['XT'].T


def monodromy_product(A, B, K, Pz0=None):
    """(A-BK)_{p-1} ... (A-BK)_0 [Pz0] as an explicit product of the closed-loop matrices."""
    Phi = np.eye(A.shape[1]) if Pz0 is None else np.array(Pz0, dtype=np.float64)
    for k in range(A.shape[0]):
        Phi = (A[k] - B[k] @ K[k]) @ Phi
    return Phi


def rho(Phi):
    return float(np.abs(np.linalg.eigvals(Phi)).max())


def telescoping_defect(A, B, H, Hc, P, K, X0, T, k0, J=None, rows=None):
    """The identity sum lc - sum l = 1/2 x_T' P_{(k0+T) mod p} x_T - 1/2 x_0' P_{k0} x_0 along the rollout -> (defect [ns], defect_rel [ns]) with the
    scale of tunempc_amd.closed_loop.cost_equivalence_batch: sum_t (|l_t| + |lc_t|) + |1/2 x_0' P x_0| + |1/2 x_T' P x_T|."""
    p = A.shape[0]
    r = rollout(A, B, K, X0, T, k0, H=H, Hc=Hc, J=J, rows=rows)
    v0 = 0.5 * np.einsum('si,ij,sj->s', X0, P[k0], X0)
    vT = 0.5 * np.einsum('si,ij,sj->s', r['XT'], P[(k0 + T) % p], r['XT'])
    defect = np.abs(r['Lc'] - r['L'] - (vT - v0))
    scale = np.abs(r['l']).sum(axis=1) + np.abs(r['lc']).sum(axis=1) + np.abs(v0) + np.abs(vT)
    return defect, defect / np.maximum(np.finfo(np.float64).tiny, scale)


def receding_horizon(A, B, H, J, rows, N, terminal='cost', Pf=None):
    """The receding-horizon loop of the horizon-N controller: K_0 from every phase (lqr_horizon_reference.horizon_lqr_phases), its monodromy on the feasible
    subspace of phase 0 -> dict K0 [p,mb,nx], Hn0 [p,nx,nx] (rows beyond c_0 zero), Phi, rho, subres = max_k max|Hn0(k+1) x_{k+1}| for the columns of Pz0(0);
    dict(infeasible=True) when a pass found no feasible subspace."""
    p, nx = A.shape[0], A.shape[1]
    res = lh.horizon_lqr_phases(A, B, H, J, rows, N, terminal, Pf)
    if any(r['infeasible'] for r in res):
        return dict(infeasible=True)
    K0 = np.stack([r['K0'] for r in res])
    Hn0 = np.zeros((p, nx, nx))
    for k, r in enumerate(res):
        Hn0[k, :r['Hn0'].shape[0]] = r['Hn0']
    x = res[0]['Pz0'].copy()
    sub = 0.0
    for k in range(p):
        x = (A[k] - B[k] @ K0[k]) @ x
        sub = max(sub, np.abs(Hn0[(k + 1) % p] @ x).max())
    return dict(infeasible=False, K0=K0, Hn0=Hn0, Phi=x, rho=rho(x), subres=sub)


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
CASES = (lh.case_no_rows, lh.case_ragged_rows, lh.case_bench_stage_shape_ragged, lh.case_single_phase)
_CACHE = {}


def with_feedback(case, ns=4, seed=11):
    """The case of lqr_horizon_reference (first problem) plus a seeded random K [p,mb,nx] (entries of the order 1 / sqrt(nx)) and X0 [ns,nx]."""
    key = (case.__name__, ns, seed)
    if key not in _CACHE:
        c = case()
        p, nx, mb = c['A'].shape[1], c['A'].shape[2], c['B'].shape[3]
        rng = np.random.default_rng(seed)
        d = {k: (None if c[k] is None else c[k][0]) for k in ('A', 'B', 'H', 'Hc', 'P', 'J', 'ncnt', 'rows')}
        d['K'] = rng.standard_normal((p, mb, nx)) / np.sqrt(nx)
        d['X0'] = rng.standard_normal((ns, nx))
        d['Hn'] = rng.standard_normal((p, nx, nx)) * (np.arange(nx)[None, :, None] < (np.arange(p) % nx)[:, None, None])      # k mod nx rows at stage k, zero below
        _CACHE[key] = d
    return _CACHE[key]


def random_batch(seed, nb, p, nx, mb, ns, nr=0, ncnt=None):
    """A seeded batch without structure (the rollout asks for none): A scaled to a spectral radius of the order one, symmetric indefinite H and Hc, a random K,
    J [nb,p,nr,n] with ncnt rows used per stage (None: all nr; ng = 0 then), Hn with k mod nx rows at stage k -> dict of contiguous arrays."""
    rng = np.random.default_rng(seed)
    n = nx + mb
    sym = lambda M: (M + np.swapaxes(M, -1, -2)) / 2
    d = dict(A=rng.standard_normal((nb, p, nx, nx)) / np.sqrt(nx), B=rng.standard_normal((nb, p, nx, mb)), K=rng.standard_normal((nb, p, mb, nx)) / np.sqrt(nx),
             X0=rng.standard_normal((nb, ns, nx)), H=sym(rng.standard_normal((nb, p, n, n))), Hc=sym(rng.standard_normal((nb, p, n, n))),
             J=rng.standard_normal((nb, p, nr, n)) if nr else None, ncnt=None if ncnt is None else np.tile(np.asarray(ncnt, np.int32), (nb, 1)))
    d['rows'] = np.full((nb, p), nr) if ncnt is None else d['ncnt'].astype(int)
    d['Hn'] = rng.standard_normal((nb, p, nx, nx)) * (np.arange(nx)[None, None, :, None] < (np.arange(p) % nx)[None, :, None, None])
    return {k: (np.ascontiguousarray(v) if v is not None else None) for k, v in d.items()}
