"""Plain-numpy statement of the inequality-constrained tracking-MPC step (test infrastructure of test_mpc_qp_cpu.py / test_gpu_mpc_qp.py; nothing under
tunempc_amd/ imports it).  For one problem, starting phase k0, initial deviation x_0 and k_j = (k0 + j) mod p:

    min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j) + 1/2 x_N' Pf_{k_N} x_N,   z_j = [x_j; u_j],
    s.t. x_{j+1} = A_k x_j + B_k u_j,   D_k z_j <= d_k (first rows_k rows),   j = 0 .. N-1.

`dense` writes it over v = [u_0 .. u_{N-1}, x_1 .. x_N] as  min 1/2 v'Qv + c'v,  Cm v = b,  G v <= h.

Method (a), `ipm`: a primal-dual interior-point method with Mehrotra's predictor-corrector on that dense problem, started infeasible.  The library runs the
same iteration stage by stage (csrc/tmpc_mpc_qp.h); the rules that define it are stated here and mirrored there:
    start      v = 0 (so x_j = 0 for j >= 1), slacks s_i = max(d_i, 1), multipliers lam_i = 1; the multipliers of the dynamics are not free variables:
               they are the adjoint of the iterate (they solve the x rows of the stationarity condition), so the dual residual lives on the u rows;
    weights    w_i = lam_i / (s_i + RHO lam_i), RHO = 1e-12: a dual regularisation that bounds the barrier weights by 1 / RHO (the stage recursion loses the
               definiteness of the cost-to-go to cancellation beyond that); its error in the row equation is RHO dlam and vanishes with the step;
    one step   length for primal and dual, alpha = min(1, 0.995 alpha_max); centring sigma = (mu_aff / mu)^3;
    stop       r_p <= tol, r_d <= tol and mu <= MU_FACTOR tol max(1, max lam), where
               r_p = max( max_i |D z + s - d|_i / max(1, |d_i|),  max|dynamics residual| / max(1, max|x|) ),
               r_d = max|u rows of the stationarity residual| / max(1, max_j |H z_j + q + D' lam_j|);
    defaults   TOL = 1e-10, MAX_ITER = 60.
Method (b), `polish`: truth.  The active set of (a) (lam > s) as equalities, one dense KKT solve, and the certificate that this is THE solution of the convex
QP: every active multiplier > 0, every inactive slack > 0, stationarity to rounding.  `margin` = min(smallest active multiplier, smallest inactive slack).

`closed_loop` is the receding-horizon loop on (b).  The cases come from lqr_horizon_reference (its Hc side, Pf = I)."""
import numpy as np

import lqr_ctg_reference as lc
import lqr_horizon_reference as lh

TOL = 1e-10
MAX_ITER = 60
MU_FACTOR = 1e-3
STEP_BACK = 0.995
RHO = 1e-12                  # dual regularisation: w = lam / (s + RHO lam) <= 1 / RHO


def dense(A, B, H, N, k0, x0, q=None, Pf=None, D=None, d=None, rows=None):
    """One problem (A [p,nx,nx], B [p,nx,mb], H [p,n,n], q [p,n], Pf [p,nx,nx], D [p,nd,n], d [p,nd], rows [p]) -> dict Q, c, Cm, b, G, h, dscale (max(1,|d_i|)
    per row of G), stage / row (of each row of G), iu, ix (index functions), N, nx, mb."""
    p, nx = A.shape[0], A.shape[1]
    mb = B.shape[2]
    nd = 0 if D is None else D.shape[1]
    if rows is None:
        rows = np.full(p, nd)
    nv = N * (mb + nx)
    iu = lambda j: slice(j * mb, (j + 1) * mb)
    ix = lambda j: slice(N * mb + (j - 1) * nx, N * mb + j * nx)            # x_j, j = 1 .. N
    Q = np.zeros((nv, nv)); c = np.zeros(nv); Cm = np.zeros((N * nx, nv)); b = np.zeros(N * nx)
    G, h, ds, st, rw = [], [], [], [], []
    for j in range(N):
        k = (k0 + j) % p
        Hk = (H[k] + H[k].T) / 2
        qk = np.zeros(nx + mb) if q is None else q[k]
        Q[iu(j), iu(j)] += Hk[nx:, nx:]
        c[iu(j)] += qk[nx:]
        if j == 0:
            c[iu(0)] += Hk[nx:, :nx] @ x0
        else:
            Q[ix(j), ix(j)] += Hk[:nx, :nx]; Q[ix(j), iu(j)] += Hk[:nx, nx:]; Q[iu(j), ix(j)] += Hk[nx:, :nx]
            c[ix(j)] += qk[:nx]
        r = slice(j * nx, (j + 1) * nx)
        Cm[r, ix(j + 1)] = np.eye(nx); Cm[r, iu(j)] = -B[k]
        if j == 0:
            b[r] = A[k] @ x0
        else:
            Cm[r, ix(j)] = -A[k]
        for i in range(int(rows[k])):
            g = np.zeros(nv)
            g[iu(j)] = D[k, i, nx:]
            hi = d[k, i]
            if j == 0:
                hi = hi - D[k, i, :nx] @ x0
            else:
                g[ix(j)] = D[k, i, :nx]
            G.append(g); h.append(hi); ds.append(max(1.0, abs(d[k, i]))); st.append(j); rw.append(i)
    if Pf is not None:
        Pn = np.asarray(Pf[(k0 + N) % p])
        Q[ix(N), ix(N)] += (Pn + Pn.T) / 2
    G = np.array(G).reshape(len(G), nv)
    return dict(Q=Q, c=c, Cm=Cm, b=b, G=G, h=np.array(h), dscale=np.array(ds), d0=np.array([d[(k0 + j) % p, i] for j, i in zip(st, rw)]), stage=np.array(st, int),
                row=np.array(rw, int), iu=iu, ix=ix, N=N, nx=nx, mb=mb, nd=nd, x0=np.asarray(x0, float))


def unpack(P, v, lam=None):
    """v (and the multipliers of the rows of G) -> X [N+1,nx], U [N,mb], Lam [N,nd]."""
    N, nx, mb = P['N'], P['nx'], P['mb']
    X = np.concatenate([P['x0'][None], v[N * mb:].reshape(N, nx)]); U = v[:N * mb].reshape(N, mb)
    Lam = np.zeros((N, P['nd']))
    if lam is not None and len(lam):
        Lam[P['stage'], P['row']] = lam
    return X, U, Lam


def ipm(P, tol=TOL, max_iter=MAX_ITER):
    """Method (a) -> dict v, lam, s, iters, status (0 converged, 1 max_iter, 2 not convex along the path, 3 non-finite), mu, rp, rd."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, m, ne = len(c), len(h), len(b)
    Nmb = P['N'] * P['mb']
    Cx = Cm[:, Nmb:]                                                        # square, block lower bidiagonal with unit diagonal
    Zn = np.concatenate([np.eye(Nmb), -np.linalg.solve(Cx, Cm[:, :Nmb])])
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0); lam = np.ones(m)
    xs0 = np.abs(P['x0']).max()
    status, it = 1, 0
    mu = rp = rd = np.nan
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            g = Q @ v + c + G.T @ lam
            nu = np.linalg.solve(Cx.T, -g[Nmb:])                             # the adjoint of the iterate
            rdv = g + Cm.T @ nu
            rpe = Cm @ v - b; rpi = G @ v + s - h
            mu = float(lam @ s) / m if m else 0.0
            rp = max(np.abs(rpi / P['dscale']).max() if m else 0.0, np.abs(rpe).max() / max(1.0, xs0, np.abs(v[Nmb:]).max()))
            rd = np.abs(rdv[:Nmb]).max() / max(1.0, np.abs(g).max())
            if not np.isfinite([mu, rp, rd]).all():
                status = 3; break
            if rp <= tol and rd <= tol and mu <= MU_FACTOR * tol * max(1.0, lam.max() if m else 0.0):
                status = 0; break
            if it == max_iter:
                break
            t = s + RHO * lam
            w = lam / t
            Kmat = np.block([[Q + G.T @ (w[:, None] * G), Cm.T], [Cm, np.zeros((ne, ne))]])
            if not np.isfinite(Kmat).all():
                status = 3; break
            red = Zn.T @ Kmat[:nv, :nv] @ Zn                                 # the Hessian on the null space of the dynamics
            if np.linalg.eigvalsh(red).min() <= 0:                           # (the library meets this as a non-positive pivot of a stage matrix S)
                status = 2; break

            def solve(corr):
                rhs = np.concatenate([-(rdv + G.T @ (corr - w * s + w * rpi)), -rpe])
                dv = np.linalg.solve(Kmat, rhs)[:nv]
                dl = corr - w * s + w * (rpi + G @ dv)
                return dv, dl, -rpi - G @ dv + RHO * dl

            def length(dl, ds):
                a = 1e300
                if m:
                    neg = ds < 0
                    if neg.any():
                        a = min(a, (-s[neg] / ds[neg]).min())
                    neg = dl < 0
                    if neg.any():
                        a = min(a, (-lam[neg] / dl[neg]).min())
                return a
            dv, dl, ds = solve(np.zeros(m))
            corr = np.zeros(m)
            if m:
                aa = min(1.0, length(dl, ds))
                sigma = (float((lam + aa * dl) @ (s + aa * ds)) / m / mu) ** 3
                corr = (sigma * mu - ds * dl) / t
                dv, dl, ds = solve(corr)
            al = min(1.0, STEP_BACK * length(dl, ds))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds
    return dict(v=v, lam=lam, s=s, iters=it, status=status, mu=mu, rp=rp, rd=rd)


def polish(P, active):
    """Method (b): the rows `active` (bool per row of G) as equalities -> dict v, lam (all rows; zero where inactive), slack = h - G v, certificate (bool),
    margin, stat (stationarity residual relative to max(1, max|gradient terms|))."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, ne = len(c), len(b)
    Ga = G[active]
    na = Ga.shape[0]
    Kmat = np.block([[Q, Cm.T, Ga.T], [Cm, np.zeros((ne, ne + na))], [Ga, np.zeros((na, ne + na))]])
    sol = np.linalg.solve(Kmat, np.concatenate([-c, b, h[active]]))
    v, nu = sol[:nv], sol[nv:nv + ne]
    lam = np.zeros(len(h)); lam[active] = sol[nv + ne:]
    slack = h - G @ v
    grad = Q @ v + c
    stat = np.abs(grad + Cm.T @ nu + G.T @ lam).max() / max(1.0, np.abs(grad).max())
    margin = min(lam[active].min() if na else np.inf, slack[~active].min() if na < len(h) else np.inf)
    return dict(v=v, lam=lam, slack=slack, stat=stat, margin=margin, certificate=bool(margin > 0 and stat <= 1e-11), nact=int(na))


def solve(A, B, H, N, k0, x0, tol=TOL, max_iter=MAX_ITER, **kw):
    """(a) then (b) on one instance -> dict a (of ipm), b (of polish), X, U, Lam of (b), Xa, Ua, Lama of (a), nact0 (active rows of stage 0), P."""
    P = dense(A, B, H, N, k0, x0, **kw)
    a = ipm(P, tol, max_iter)
    act = a['lam'] > a['s']
    bb = polish(P, act)
    X, U, Lam = unpack(P, bb['v'], bb['lam'])
    Xa, Ua, Lama = unpack(P, a['v'], a['lam'])
    return dict(a=a, b=bb, X=X, U=U, Lam=Lam, Xa=Xa, Ua=Ua, Lama=Lama, nact0=int((act & (P['stage'] == 0)).sum()), P=P)


def closed_loop(A, B, H, N, k0, x0, T, **kw):
    """The receding-horizon loop on (b): at t the QP from phase (k0 + t) mod p, u_0 applied to the linear plant -> dict X [T+1,nx], U [T,mb], nact [T] (stage 0), nact_all [T] (whole horizon), hres [T]
    (max(D z - d) of the applied step; -inf at a stage without rows), margin (smallest over the steps), certificate (all steps)."""
    p, nx = A.shape[0], A.shape[1]
    D, d, rows = kw.get('D'), kw.get('d'), kw.get('rows')
    X = [np.asarray(x0, float)]; U = []; nact = []; nall = []; hres = []; margin = np.inf; cert = True
    for t in range(T):
        k = (k0 + t) % p
        r = solve(A, B, H, N, k, X[-1], **kw)
        u = r['U'][0]
        z = np.concatenate([X[-1], u])
        rk = 0 if D is None else int(D.shape[1] if rows is None else rows[k])
        hres.append((D[k, :rk] @ z - d[k, :rk]).max() if rk else -np.inf)
        U.append(u); nact.append(r['nact0']); nall.append(r['b']['nact']); margin = min(margin, r['b']['margin']); cert = cert and r['b']['certificate'] and r['a']['status'] == 0
        X.append(A[k] @ X[-1] + B[k] @ u)
    return dict(X=np.array(X), U=np.array(U), nact=np.array(nact), nact_all=np.array(nall), hres=np.array(hres), margin=margin, certificate=cert)


def kkt_check(A, B, H, N, k0, X, U, Lam, q=None, Pf=None, D=None, d=None, rows=None):
    """Solver-independent figures of a returned open-loop solution, each relative to its natural scale: dict dyn (dynamics residual / max(1, max|X|)),
    viol (max(D z - d) / max(1, |d|), <= 0 up to rounding when feasible), lam_min, comp (max |lam (d - D z)| / max(1, max lam)), stat (the u rows of the
    stationarity condition with the adjoint pi_j = (H z_j + q + D' lam_j)_x + A' pi_{j+1}, pi_N = Pf x_N, relative to max(1, max|H z + q + D' lam|))."""
    p, nx = A.shape[0], A.shape[1]
    dyn = viol = comp = stat = gmax = 0.0
    lam_min = np.inf
    pi = np.zeros(nx) if Pf is None else ((Pf[(k0 + N) % p] + Pf[(k0 + N) % p].T) / 2) @ X[N]
    for j in range(N - 1, -1, -1):
        k = (k0 + j) % p
        z = np.concatenate([X[j], U[j]])
        E = np.concatenate([A[k], B[k]], axis=1)
        dyn = max(dyn, np.abs(E @ z - X[j + 1]).max())
        g = ((H[k] + H[k].T) / 2) @ z + (0 if q is None else q[k])
        rk = 0 if D is None else int(D.shape[1] if rows is None else rows[k])
        if rk:
            lam = Lam[j, :rk]
            g = g + D[k, :rk].T @ lam
            r = D[k, :rk] @ z - d[k, :rk]
            viol = max(viol, (r / np.maximum(1.0, np.abs(d[k, :rk]))).max())
            comp = max(comp, np.abs(lam * r).max()); lam_min = min(lam_min, lam.min())
        gmax = max(gmax, np.abs(g).max())
        full = g + E.T @ pi
        stat = max(stat, np.abs(full[nx:]).max())
        pi = full[:nx]
    lmax = max(1.0, np.abs(Lam).max()) if Lam.size else 1.0
    return dict(dyn=dyn / max(1.0, np.abs(X).max()), viol=viol, lam_min=lam_min, comp=comp / lmax, stat=stat / max(1.0, gmax))


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def _unconstrained_u0(c, N, X0, k0):
    A, B, H = c['A'][0], c['B'][0], c['H'][0]
    out = []
    for x0 in X0:
        P = dense(A, B, H, N, k0, x0, Pf=c['Pf'][0])
        out.append(polish(P, np.zeros(0, bool))['v'][:B.shape[2]])
    return np.array(out)


def _finish(name, base, N, k0, ns, seed, box=None, mixed=None, q_scale=0.0):
    """base: a case of lqr_horizon_reference (its Hc is the positive definite side).  box: factor of the largest unconstrained |u_0| -> rows +-u <= umax;
    mixed: (counts per stage, d) -> random rows on [x; u]."""
    if name in _CACHE:
        return _CACHE[name]
    A, B, H = base['A'], base['B'], base['Hc']
    nb, p, nx, _ = A.shape
    mb = B.shape[3]
    n = nx + mb
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal((nb, ns, nx))
    c = dict(A=A, B=B, H=H, Pf=np.ascontiguousarray(np.broadcast_to(np.eye(nx), (nb, p, nx, nx))), X0=X0, N=N, k0=k0, q=None, ncnt=None)
    if box is not None:
        umax = box * np.abs(_unconstrained_u0(c, N, X0[0], k0)).max()
        D = np.zeros((nb, p, 2 * mb, n))
        D[:, :, :mb, nx:] = np.eye(mb); D[:, :, mb:, nx:] = -np.eye(mb)
        c.update(D=D, d=np.full((nb, p, 2 * mb), umax), rows=np.full((nb, p), 2 * mb), umax=umax)
    else:
        counts, dval = mixed
        nd = max(counts)
        D = np.zeros((nb, p, nd, n)); d = np.zeros((nb, p, nd))
        for k in range(p):
            D[:, k, :counts[k]] = rng.standard_normal((nb, counts[k], n)); d[:, k, :counts[k]] = dval * (1 + rng.random((nb, counts[k])))
        c.update(D=D, d=d, rows=np.tile(np.asarray(counts), (nb, 1)), ncnt=np.tile(np.asarray(counts, np.int32), (nb, 1)))
    if q_scale:
        c['q'] = q_scale * rng.standard_normal((nb, p, n))
    _CACHE[name] = c
    return c


def _bench_base():
    if 'bench_base' not in _CACHE:
        A, B, Hc, _ = lc.gen_problem(7, 1, 2, 24, 8, 0)
        _CACHE['bench_base'] = dict(A=A, B=B, Hc=Hc)
    return _CACHE['bench_base']


def case_box_nu1():
    """p 3 / nx 3 / nu 1, N = 5 > p from phase 2 (the phase wraps), input box at half the largest unconstrained |u_0|."""
    return _finish('box_nu1', lh.case_no_rows(), 5, 2, 4, 11, box=0.5)


def case_box_nu2():
    """p 3 / nx 3 / nu 2, N = 4, input box."""
    return _finish('box_nu2', lh.case_ragged_rows(), 4, 0, 4, 12, box=0.5)


def case_box_bench():
    """The bench stage shape p 2 / nx 24 / nu 8, N = 6, the 16-row input box."""
    return _finish('box_bench', _bench_base(), 6, 1, 3, 13, box=0.5)


def case_mixed_small(N=4):
    """p 3 / nx 3 / nu 2, ragged random rows on [x; u] (2, 0, 1 per stage), q != 0, N = 4 (or N = 2 < p)."""
    return _finish('mixed_small_%d' % N, lh.case_ragged_rows(), N, 1, 4, 14, mixed=([2, 0, 1], 0.4), q_scale=0.3)


def case_mixed_bench():
    """The bench stage shape with 6 / 3 random rows, q != 0."""
    return _finish('mixed_bench', _bench_base(), 6, 0, 3, 15, mixed=([6, 3], 1.5), q_scale=0.3)


def case_single_phase():
    """p 1 / nx 3 / nu 2, N = 3, input box."""
    return _finish('p1', lh.case_single_phase(), 3, 0, 3, 16, box=0.5)


def case_layout_edge():
    """nx 40 / nu 24 with 4 rows, N = 2: the edge of the LDS layout."""
    if 'edge_base' not in _CACHE:
        A, B, Hc, _ = lc.gen_problem(9, 1, 2, 40, 24, 0)
        _CACHE['edge_base'] = dict(A=A, B=B, Hc=Hc)
    return _finish('edge', _CACHE['edge_base'], 2, 0, 2, 17, mixed=([4, 4], 3.0))


CASES = [case_box_nu1, case_box_nu2, case_box_bench, case_mixed_small, case_mixed_bench, case_single_phase, case_layout_edge]


def kwargs(c, b=0):
    """The keyword arguments of dense / solve / closed_loop for member b of a case."""
    return dict(q=None if c['q'] is None else c['q'][b], Pf=c['Pf'][b], D=c['D'][b], d=c['d'][b], rows=c['rows'][b])


def solve_case(c):
    """Every instance of a case through (a) and (b), once per process -> list [nb][ns] of the dicts of `solve`."""
    key = ('solved', id(c))
    if key not in _CACHE:
        _CACHE[key] = [[solve(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, **kwargs(c, b)) for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]
    return _CACHE[key]


def ab_disagreement(r):
    """(a) against (b) on one instance: the whole solution, u_0 and the multipliers, relative to max(1, max|.|) of (b)."""
    rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max()) if y.size else 0.0
    return dict(sol=max(rel(r['Xa'], r['X']), rel(r['Ua'], r['U'])), u0=rel(r['Ua'][0], r['U'][0]), lam=rel(r['Lama'], r['Lam']))
