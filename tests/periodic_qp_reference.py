"""Plain-numpy statement of the PERIODIC optimal-control QP (the LQ case of the reference's pocp.py, the subproblem of its sqp_method.Sqp): test
infrastructure of test_periodic_qp_cpu.py / test_gpu_periodic_qp*.py.  Per problem, with N = periods p and k_j = j mod p,

    min   sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j),   z_j = [x_j; u_j],
    s.t.  x_{j+1} = A_k x_j + B_k u_j + c_k,  j = 0 .. N-1,  x_N := x_0  (x_0 is a variable),
          D_k z_j <= d_k (first rows_k rows),   J_k z_j = r_k (first erows_k rows).

`dense` states it over v = [x_0 .. x_{N-1}, u_0 .. u_{N-1}] as  min 1/2 v' Q v + c' v,  Cm v = b,  G v <= h,  Je v = re; the cyclic dynamics rows are
the rows of Cm (block j: A_k x_j + B_k u_j - x_{(j+1) mod N} = -c_k).

Method (a), `ipm`: the hard / equality-row iteration of mpc_qp_eq_reference.ipm_eq on the dense problem.  The library runs the same iteration stage by
stage (csrc/tmpc_periodic_qp.h); the rules, stated here and mirrored there:
    start      v = 0 (x_0 included), s = max(d, 1), lam = 1, nu = 0, pi_per = 0;
    weights    w = lam / (s + RHO lam) on an inequality row, the constant 1 / RHO on an equality row;
    multipliers of the dynamics: pi_per, the multiplier of x_N = x_0 (block N-1 of Cm), is a VARIABLE -- I - (A_{N-1} .. A_0)' may be singular, so it
               cannot be derived from the iterate.  The others are the adjoint of the iterate started from it:
               pi_j = (H z_j + q + D' lam_j + J' nu_j)_x + A_j' pi_{j+1},  j = N-1 .. 1,  pi_N = pi_per;
    residuals  dual: the u rows of every stage and the x_0 rows (H z_0 + q + D' lam + J' nu)_x + A_0' pi_1 - pi_per; the dynamics residual of the last
               stage is E z_{N-1} + c - x_0;
    Newton     one linear system per predictor and per corrector, Mehrotra with sigma = (mu_aff / mu)^3, one step length 0.995 alpha_max for everything
               (pi_per moves with it); the library solves the system by a Riccati pass plus a border of nx columns and a quasi-definite system of
               size 2 nx (`newton_border` restates that elimination; `newton_dense` is the same direction from the dense KKT matrix);
    stop       r_p <= tol, r_d <= tol, mu <= 1e-3 tol max(1, max lam) with r_p = max(max|r_in| / max(1, |d|), max|J z - r| / max(1, |r|),
               max|r_dyn| / max(1, max|x|)), r_d = max|dual residual| / max(1, max|H z + q + D' lam + J' nu|);
    statuses   0 converged, 1 max_iter, 2 the Newton system has no unique solution (a reduced Hessian that is not positive definite, or dynamics rows that
               are dependent: no periodic trajectory, e.g. A = I, B = 0, c != 0), 3 non-finite.
Method (b), `polish`: truth.  The active set of (a) (lam > s) as equalities and one dense KKT solve; the certificate is: active multipliers > 0, inactive
slacks > 0 (their smallest is `margin`), stationarity and the equalities to rounding."""
import numpy as np

import mpc_qp_reference as mq
import mpc_qp_soft_reference as sq

TOL, MAX_ITER, RHO = mq.TOL, mq.MAX_ITER, mq.RHO
MARGIN_MIN = sq.MARGIN_MIN
# (a) against (b) over every feasible case below: X, U relative to max(1, max|.|) of (b), lam, nu, pi relative to max(1, max lam, max|nu|, max|pi|) of (b).
# Measured 9.2e-12, on lam of stage_shape (test_periodic_qp_cpu.py prints every figure and asserts the bound); rounded up to one digit.
PER_IPM_VS_POLISH = 1e-11
PARITY = 10 * PER_IPM_VS_POLISH      # the GPU tests: the project's margin for another order of accumulation on the device


def dense(A, B, H, periods=1, q=None, c=None, D=None, d=None, rows=None, J=None, r=None, erows=None):
    """A [p,nx,nx], B [p,nx,nu], H [p,n,n]; q [p,n], c [p,nx], D [p,nd,n], d [p,nd], rows [p], J [p,ne,n], r [p,ne], erows [p] (None: zero / all rows).
    -> dict Q, c, Cm, b, G, h, d0, dscale, stage, row, Je, re, escale, estage, erow, N, nx, mb, nd, ne, ix, iu, stages (per j: E, H, q, c, D, d, J, r)."""
    A, B, H = (np.asarray(x, float) for x in (A, B, H))
    p, nx, mb = A.shape[0], A.shape[1], B.shape[2]
    n, N = nx + mb, periods * p
    nv = N * n
    ix = lambda j: slice(j * nx, (j + 1) * nx)
    iu = lambda j: slice(N * nx + j * mb, N * nx + (j + 1) * mb)
    nd = 0 if D is None else D.shape[1]
    ne = 0 if J is None else J.shape[1]
    Q = np.zeros((nv, nv)); cv = np.zeros(nv); Cm = np.zeros((N * nx, nv)); b = np.zeros(N * nx)
    G, h, st, rw, Je, re, es, est, erw, stages = [], [], [], [], [], [], [], [], [], []
    for j in range(N):
        k = j % p
        Hs = 0.5 * (H[k] + H[k].T)
        sel = np.r_[np.arange(j * nx, (j + 1) * nx), np.arange(N * nx + j * mb, N * nx + (j + 1) * mb)]
        Q[np.ix_(sel, sel)] += Hs
        qk = np.zeros(n) if q is None else np.asarray(q[k], float)
        ck = np.zeros(nx) if c is None else np.asarray(c[k], float)
        cv[sel] += qk
        rb = slice(j * nx, (j + 1) * nx)
        Cm[rb, ix(j)] += A[k]; Cm[rb, iu(j)] += B[k]; Cm[rb, ix((j + 1) % N)] -= np.eye(nx)
        b[rb] = -ck
        m = 0 if D is None else int(nd if rows is None else rows[k])
        me = 0 if J is None else int(ne if erows is None else erows[k])
        for i in range(m):
            g = np.zeros(nv); g[sel] = D[k, i]
            G.append(g); h.append(d[k, i]); st.append(j); rw.append(i)
        for i in range(me):
            g = np.zeros(nv); g[sel] = J[k, i]
            ri = 0.0 if r is None else r[k, i]
            Je.append(g); re.append(ri); es.append(max(1.0, abs(ri))); est.append(j); erw.append(i)
        stages.append(dict(E=np.concatenate([A[k], B[k]], axis=1), H=Hs, q=qk, c=ck, D=np.zeros((0, n)) if not m else np.asarray(D[k, :m], float),
                           d=np.zeros(0) if not m else np.asarray(d[k, :m], float), J=np.zeros((0, n)) if not me else np.asarray(J[k, :me], float),
                           r=np.zeros(me) if (r is None or not me) else np.asarray(r[k, :me], float), sel=sel))
    h = np.array(h, float)
    return dict(Q=Q, c=cv, Cm=Cm, b=b, G=np.array(G).reshape(len(G), nv), h=h, d0=h.copy(), dscale=np.maximum(1.0, np.abs(h)), stage=np.array(st, int),
                row=np.array(rw, int), Je=np.array(Je).reshape(len(Je), nv), re=np.array(re, float), escale=np.array(es, float), estage=np.array(est, int),
                erow=np.array(erw, int), N=N, nx=nx, mb=mb, nd=nd, ne=ne, ix=ix, iu=iu, stages=stages)


def unpack(P, v, lam=None, nue=None, piv=None):
    """-> X [N,nx], U [N,nu], Lam [N,nd], Nu [N,ne], Pi [N,nx] (Pi[0]: the multiplier of x_N = x_0, Pi[j]: that of x_j = E z_{j-1} + c)."""
    N, nx, mb = P['N'], P['nx'], P['mb']
    X = v[:N * nx].reshape(N, nx).copy(); U = v[N * nx:].reshape(N, mb).copy()
    Lam = np.zeros((N, P['nd'])); Nu = np.zeros((N, P['ne'])); Pi = np.zeros((N, nx))
    if lam is not None and len(lam):
        Lam[P['stage'], P['row']] = lam
    if nue is not None and len(nue):
        Nu[P['estage'], P['erow']] = nue
    if piv is not None:
        Pi = np.roll(np.asarray(piv, float).reshape(N, nx), 1, axis=0)
    return X, U, Lam, Nu, Pi


def adjoint(P, g, piper):
    """The multipliers of the N blocks of Cm from pi_per (block N-1) and the gradient g of the iterate: block j-1 = g_{x_j} + A_j' block j."""
    N, nx = P['N'], P['nx']
    piv = np.zeros((N, nx)); piv[N - 1] = piper
    for j in range(N - 1, 0, -1):
        piv[j - 1] = g[P['ix'](j)] + P['stages'][j]['E'][:, :nx].T @ piv[j]
    return piv.reshape(-1)


def newton_dense(P, v, lam, s, nue, piper, c1, augmented=False):
    """The Newton direction at an iterate from the dense KKT matrix -> dv, dlam, ds, dnue, dpi_per, or None when the system has no unique solution.
    augmented: the same system with dnue as an unknown, its rows [Je, -RHO I] kept as rows: no 1 / RHO stands in the matrix, and dnue is not formed as
    the difference Je dv + req blown up by 1 / RHO (the truth path of tests/qp_path_reference.py)."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, nq, me = len(c), len(b), len(re)
    g = Q @ v + c + G.T @ lam + Je.T @ nue
    rdv = g + Cm.T @ adjoint(P, g, piper)
    rpe = Cm @ v - b; rpi = G @ v + s - h; req = Je @ v - re
    w = lam / (s + RHO * lam)
    Hb = Q + G.T @ (w[:, None] * G) + Je.T @ Je / RHO
    Kmat = np.block([[Hb, Cm.T], [Cm, np.zeros((nq, nq))]])
    if not np.isfinite(Kmat).all():
        return None
    _, sv, Vt = np.linalg.svd(Cm)
    if sv.min() <= 1e-12 * sv.max():
        return None
    Zn = Vt[nq:].T
    if Zn.shape[1] and np.linalg.eigvalsh(Zn.T @ Hb @ Zn).min() <= 0:
        return None
    beta = rpi - s + c1 / lam
    if augmented:
        Kaug = np.block([[Q + G.T @ (w[:, None] * G), Cm.T, Je.T], [Cm, np.zeros((nq, nq + me))], [Je, np.zeros((me, nq)), -RHO * np.eye(me)]])
        sol = np.linalg.solve(Kaug, np.concatenate([-(rdv + G.T @ (w * beta)), -rpe, -req]))
        dv, dn = sol[:nv], sol[nv + nq:]
        dl = w * (beta + G @ dv)
        return dv, dl, -rpi - G @ dv + RHO * dl, dn, sol[nv:nv + nq][-P['nx']:]
    sol = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta) + Je.T @ (req / RHO)), -rpe]))
    dv = sol[:nv]
    dl = w * (beta + G @ dv)
    return dv, dl, -rpi - G @ dv + RHO * dl, (Je @ dv + req) / RHO, sol[nv:][-P['nx']:]


def newton_border(P, v, lam, s, nue, piper, c1):
    """The same direction the way csrc/tmpc_periodic_qp.h eliminates it: the Riccati pass from Pi_N = 0, p_N = pi_per; nx border columns M_j = Phi_{N<-j}'
    swept backward with its factors (M_N = I, T = E' M_{j+1}, Gy_j = R^-T T_u, M_j = T_x - Y' Gy_j), Gamma = sum Gy_j' Gy_j and
    phi = sum (M_{j+1}' r_dyn_j - Gy_j' y_j) accumulated along; then, with a = p_0 - pi_per,
        [ Pi_0       M_0 - I ] [dx_0]     [ a   ]
        [ M_0' - I   -Gamma  ] [dpi ] = - [ phi ]
    by Pi_0 = R0' R0, W = R0^-T (M_0 - I), (Gamma + W' W) dpi = phi - W' R0^-T a, dx_0 = -R0^-1 (R0^-T a + W dpi); the forward sweep
    du = -R^-1 (Y dx + y + Gy dpi), dx+ = E dz + r_dyn.  -> dv, dpi, pivots: the elimination pivots the kernel feeds to pivmin, the squares of the
    diagonals of (the R of the stages j = N-1 .. 0, one array; R0 then R2, one array): the first set belongs to pass 1 of the iterate, the second to
    the border system that only an iterate that takes a step factors; rows: (dlam, ds, dnue) from the forward sweep, stage by stage, with the residuals
    r_in and r_eq that entered the right-hand side: dlam = w (r_in - s + c1 / lam + D dz), ds = -r_in - D dz + RHO dlam, dnu = (1 / RHO)(J dz + r_eq)."""
    N, nx, mb = P['N'], P['nx'], P['mb']
    X, U, _, _, _ = unpack(P, v)
    w = lam / (s + RHO * lam)
    Pi = np.zeros((nx, nx)); pv = np.array(piper, float); M = np.eye(nx); Gam = np.zeros((nx, nx)); phi = np.zeros(nx)
    fac = [None] * N
    spiv = []
    for j in range(N - 1, -1, -1):
        S = P['stages'][j]
        E, z = S['E'], np.concatenate([X[j], U[j]])
        gi, ei = P['stage'] == j, P['estage'] == j
        lj, sj, wj, cj = lam[gi], s[gi], w[gi], c1[gi]
        rin = S['D'] @ z + sj - S['d']; rdyn = E @ z + S['c'] - X[(j + 1) % N]; rq = S['J'] @ z - S['r']
        Hb = S['H'] + E.T @ Pi @ E + S['D'].T @ (wj[:, None] * S['D']) + S['J'].T @ S['J'] / RHO
        hh = S['H'] @ z + S['q'] + S['D'].T @ (wj * (rin + RHO * lj) + wj * cj / lj) + S['J'].T @ (nue[ei] + rq / RHO) + E.T @ (Pi @ rdyn + pv)
        R = np.linalg.cholesky(Hb[nx:, nx:]).T
        Y = np.linalg.solve(R.T, Hb[nx:, :nx]); y = np.linalg.solve(R.T, hh[nx:])
        T = E.T @ M
        Gy = np.linalg.solve(R.T, T[nx:])
        phi = phi + M.T @ rdyn - Gy.T @ y
        Gam = Gam + Gy.T @ Gy
        M = T[:nx] - Y.T @ Gy
        Pi = 0.5 * (Hb[:nx, :nx] + Hb[:nx, :nx].T) - Y.T @ Y
        pv = hh[:nx] - Y.T @ y
        fac[j] = (R, Y, y, Gy, rdyn, rin, rq)
        spiv.append(np.diag(R) ** 2)
    a = pv - piper
    R0 = np.linalg.cholesky(Pi).T
    W = np.linalg.solve(R0.T, M - np.eye(nx)); wv = np.linalg.solve(R0.T, a)
    R2 = np.linalg.cholesky(Gam + W.T @ W).T
    dpi = np.linalg.solve(R2, np.linalg.solve(R2.T, phi - W.T @ wv))
    dx = -np.linalg.solve(R0, wv + W @ dpi)
    dX = np.zeros((N, nx)); dU = np.zeros((N, mb))
    dl = np.zeros(len(lam)); ds = np.zeros(len(lam)); dn = np.zeros(len(nue))
    for j in range(N):
        R, Y, y, Gy, rdyn, rin, rq = fac[j]
        S = P['stages'][j]
        du = -np.linalg.solve(R, Y @ dx + y + Gy @ dpi)
        dX[j], dU[j] = dx, du
        dz = np.concatenate([dx, du])
        gi, ei = P['stage'] == j, P['estage'] == j
        Dz = S['D'] @ dz
        dl[gi] = w[gi] * (rin - s[gi] + c1[gi] / lam[gi] + Dz)
        ds[gi] = -rin - Dz + RHO * dl[gi]
        dn[ei] = (S['J'] @ dz + rq) / RHO
        dx = S['E'] @ dz + rdyn
    return np.concatenate([dX.reshape(-1), dU.reshape(-1)]), dpi, (np.concatenate(spiv), np.concatenate([np.diag(R0) ** 2, np.diag(R2) ** 2])), (dl, ds, dn)


def newton_staged(P, v, lam, s, nue, piper, c1, reuse=True):
    """newton_border as the tuple of newton_dense -> dv, dlam, ds, dnue, dpi_per.  reuse=True: the rows of its forward sweep, as the kernel computes them.
    reuse=False: dlam, ds, dnue by the same formulas from residuals G v + s - h and Je v - re EVALUATED AGAIN on the dense problem.  They differ from the
    residuals inside the right-hand side by one rounding (another order of summation), 1e-16, and the formulas multiply that by w <= 1 / RHO = 1e12: the
    multipliers then carry a noise of 1e-4 that no later step removes, and r_d stalls there (test_qp_path_cpu.py shows both)."""
    dv, dpi, _, rows = newton_border(P, v, lam, s, nue, piper, c1)
    if reuse:
        return (dv,) + rows + (dpi,)
    G, h, Je, re = (P[k] for k in ('G', 'h', 'Je', 're'))
    w = lam / (s + RHO * lam)
    rpi = G @ v + s - h
    dl = w * (rpi - s + c1 / lam + G @ dv)
    return dv, dl, -rpi - G @ dv + RHO * dl, (Je @ dv + (Je @ v - re)) / RHO, dpi


def ipm(P, tol=TOL, max_iter=MAX_ITER, augmented=False, staged=False, pivots=False, reuse=True):
    """Method (a) -> dict v, lam, s, nue, pi (the N blocks of Cm), piper, iters, status, mu, rp, rd.  augmented: the directions from newton_dense(augmented=True);
    staged: from newton_staged(reuse=reuse) (the kernel's elimination) -- the iteration and its rules are the same, only the linear algebra of the step differs.  pivots: also
    pivmin, the smallest elimination pivot of newton_border the way the kernel collects it: over pass 1 of every iterate reached, the last included, and over
    the border systems of the iterates that took a step."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, m, nx, Nnx = len(c), len(h), P['nx'], P['N'] * P['nx']
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0) if m else np.zeros(0); lam = np.ones(m); nue = np.zeros(len(re)); piper = np.zeros(nx)
    status, it = 1, 0
    mu = rp = rd = np.nan
    piv = np.zeros(Nnx)
    pivmin = np.inf
    if staged:
        newton = lambda *a: newton_staged(P, *a, reuse=reuse)
    else:
        newton = lambda *a: newton_dense(P, *a, augmented=augmented)
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            if pivots:
                _, _, (spiv, bpiv), _ = newton_border(P, v, lam, s, nue, piper, np.zeros(m))
                pivmin = min(pivmin, spiv.min())
            g = Q @ v + c + G.T @ lam + Je.T @ nue
            piv = adjoint(P, g, piper)
            rdv = g + Cm.T @ piv
            rpe = Cm @ v - b; rpi = G @ v + s - h; req = Je @ v - re
            mu = float(lam @ s) / m if m else 0.0
            xsc = max(1.0, np.abs(v[:Nnx]).max())
            rp = max(np.abs(rpi / P['dscale']).max() if m else 0.0, np.abs(rpe).max() / xsc, np.abs(req / P['escale']).max() if len(re) else 0.0)
            rd = np.abs(rdv).max() / max(1.0, np.abs(g).max())
            lmax = lam.max() if m else 0.0
            if not np.isfinite([mu, rp, rd, lmax, xsc]).all():
                status = 3; break
            if rp <= tol and rd <= tol and mu <= mq.MU_FACTOR * tol * max(1.0, lmax):
                status = 0; break
            if it == max_iter:
                break
            if not (np.isfinite(Q).all() and np.isfinite(Cm).all() and np.isfinite(G).all() and np.isfinite(Je).all()):
                status = 3; break
            step = newton(v, lam, s, nue, piper, np.zeros(m))
            if step is None:
                status = 2; break
            if pivots:
                pivmin = min(pivmin, bpiv.min())

            def length(dl, ds):
                a = 1e300
                for x, dx in ((s, ds), (lam, dl)):
                    neg = dx < 0
                    if neg.any():
                        a = min(a, (-x[neg] / dx[neg]).min())
                return a
            dv, dl, ds, dn, dp = step
            if m:
                aa = min(1.0, length(dl, ds))
                sigmu = (float((lam + aa * dl) @ (s + aa * ds)) / m / mu) ** 3 * mu
                dv, dl, ds, dn, dp = newton(v, lam, s, nue, piper, sigmu - ds * dl)
            al = min(1.0, mq.STEP_BACK * length(dl, ds))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; nue = nue + al * dn; piper = piper + al * dp
    out = dict(v=v, lam=lam, s=s, nue=nue, pi=piv, piper=piper, iters=it, status=status, mu=mu, rp=rp, rd=rd)
    if pivots:
        out['pivmin'] = pivmin
    return out


def polish(P, active):
    """Method (b) -> dict v, lam, nue, pi, slack, stat, eqres, margin, certificate, nact."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, nq, me = len(c), len(b), len(re)
    act = np.asarray(active, bool)
    Ga = G[act]
    na = Ga.shape[0]
    rowsm = np.vstack([Cm, Je, Ga])
    K = np.block([[Q, rowsm.T], [rowsm, np.zeros((len(rowsm), len(rowsm)))]])
    sol = np.linalg.solve(K, np.concatenate([-c, b, re, h[act]]))
    v, piv, nue = sol[:nv], sol[nv:nv + nq], sol[nv + nq:nv + nq + me]
    lam = np.zeros(len(h)); lam[act] = sol[nv + nq + me:]
    slack = h - G @ v
    grad = Q @ v + c
    stat = np.abs(grad + Cm.T @ piv + G.T @ lam + Je.T @ nue).max() / max(1.0, np.abs(grad).max())
    eqres = max(np.abs(Je @ v - re).max() if me else 0.0, np.abs(Cm @ v - b).max(), np.abs(slack[act]).max() if na else 0.0)
    strict = [slack[~act], lam[act]]
    margin = min([x.min() for x in strict if x.size] + [np.inf])
    cert = bool(margin > 0 and stat <= 1e-11 and eqres <= 1e-11 * max(1.0, np.abs(v).max()))
    return dict(v=v, lam=lam, nue=nue, pi=piv, slack=slack, stat=stat, eqres=eqres, margin=margin, certificate=cert, nact=int(na), active=act)


def solve(A, B, H, periods=1, tol=TOL, max_iter=MAX_ITER, **kw):
    """(a) then (b) on one problem -> dict a, b, P, X, U, Lam, Nu, Pi, cost of (b), Xa, Ua, Lama, Nua, Pia of (a), active [N, nd] bool."""
    P = dense(A, B, H, periods, **kw)
    a = ipm(P, tol, max_iter)
    out = dict(a=a, P=P)
    out['Xa'], out['Ua'], out['Lama'], out['Nua'], out['Pia'] = unpack(P, a['v'], a['lam'], a['nue'], a['pi'])
    if a['status'] == 0:
        bb = polish(P, a['lam'] > a['s'])
        out['b'] = bb
        out['X'], out['U'], out['Lam'], out['Nu'], out['Pi'] = unpack(P, bb['v'], bb['lam'], bb['nue'], bb['pi'])
        out['cost'] = float(0.5 * bb['v'] @ P['Q'] @ bb['v'] + P['c'] @ bb['v'])
        act = np.zeros((P['N'], P['nd']), bool)
        if len(P['h']):
            act[P['stage'], P['row']] = bb['active']
        out['active'] = act
    return out


def mult_scale(r):
    return max([1.0] + [np.abs(r[k]).max() for k in ('Lam', 'Nu', 'Pi') if r[k].size])


def ab_disagreement(r):
    """(a) against (b): X, U relative to max(1, max|.|) of (b); lam, nu, pi relative to max(1, max lam, max|nu|, max|pi|) of (b)."""
    rel = lambda x, y, sc: np.abs(x - y).max() / sc if y.size else 0.0
    ls = mult_scale(r)
    return dict(sol=max(rel(r['Xa'], r['X'], max(1.0, np.abs(r['X']).max())), rel(r['Ua'], r['U'], max(1.0, np.abs(r['U']).max()))),
                lam=rel(r['Lama'], r['Lam'], ls), nu=rel(r['Nua'], r['Nu'], ls), pi=rel(r['Pia'], r['Pi'], ls))


def scalar_closed_form(a, b, c, H, q, umax=None):
    """nx = nu = p = N = 1: (1 - a) x = b u + c.  Substituting x = al u + be into the cost, the stationarity of the one-variable quadratic gives u; with the
    bound u <= umax active, u = umax.  -> x, u, active."""
    al, be = b / (1.0 - a), c / (1.0 - a)
    u = -(al * H[0, 0] * be + H[0, 1] * be + al * q[0] + q[1]) / (al * al * H[0, 0] + 2.0 * al * H[0, 1] + H[1, 1])
    active = umax is not None and u > umax
    if active:
        u = umax
    return al * u + be, u, bool(active)


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def _model(seed, nx, nu, p, radius=0.9):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((p, nx, nx))
    for k in range(p):
        A[k] *= radius / max(abs(np.linalg.eigvals(A[k])))
    B = rng.standard_normal((p, nx, nu))
    M = rng.standard_normal((p, nx + nu, nx + nu))
    H = np.einsum('kij,klj->kil', M, M) / (nx + nu) + np.eye(nx + nu)
    return A, B, H, rng.standard_normal((p, nx + nu)), 0.5 * rng.standard_normal((p, nx))


def _rows(seed, A, B, H, q, c, counts, ecounts, periods=1, every=2):
    """Random rows: equality rows J z = r with a small r; inequality rows whose right-hand side is set around the optimum WITHOUT them, every `every`-th
    one 0.2 inside it (the row becomes active) and the others 0.5 beyond it (inactive)."""
    rng = np.random.default_rng(seed)
    p, n = A.shape[0], H.shape[1]
    nd, ne = max(counts), max(ecounts)
    J = np.zeros((p, ne, n)); r = np.zeros((p, ne)); D = np.zeros((p, nd, n)); d = np.zeros((p, nd))
    for k in range(p):
        J[k, :ecounts[k]] = rng.standard_normal((ecounts[k], n)); r[k, :ecounts[k]] = 0.1 * rng.standard_normal(ecounts[k])
        Dk = rng.standard_normal((counts[k], n))
        D[k, :counts[k]] = Dk / np.linalg.norm(Dk, axis=1, keepdims=True) if counts[k] else Dk
    kw = dict(q=q, c=c, J=J if ne else None, r=r if ne else None, erows=np.asarray(ecounts) if ne else None)
    P = dense(A, B, H, periods, **kw)
    free = polish(P, np.zeros(0, bool))
    X, U, _, _, _ = unpack(P, free['v'])
    t = 0
    for k in range(p):
        z = np.concatenate([X[k], U[k]])
        for i in range(counts[k]):
            d[k, i] = D[k, i] @ z + (-0.2 if t % every == 0 else 0.5)
            t += 1
    kw.update(D=D if nd else None, d=d if nd else None, rows=np.asarray(counts) if nd else None)
    return kw


def _box(A, B, H, q, c, frac):
    """The input box |u_i| <= frac max|u| of the orbit without rows, at every stage (2 nu rows)."""
    p, nx, nu = B.shape
    P = dense(A, B, H, 1, q=q, c=c)
    _, U, _, _, _ = unpack(P, polish(P, np.zeros(0, bool))['v'])
    umax = frac * np.abs(U).max()
    D = np.zeros((p, 2 * nu, nx + nu)); D[:, :nu, nx:] = np.eye(nu); D[:, nu:, nx:] = -np.eye(nu)
    return dict(q=q, c=c, D=D, d=np.full((p, 2 * nu), umax), rows=None)


def _case(name, make):
    if name not in _CACHE:
        A, B, H, periods, kw = make()
        _CACHE[name] = dict(name=name, A=A, B=B, H=H, periods=periods, kw=kw)
    return _CACHE[name]


SCALAR = dict(a=0.7, b=1.2, c=0.5, H=np.array([[2.0, 0.3], [0.3, 1.0]]), q=np.array([-1.0, -2.0]))


def _scalar(umax):
    s = SCALAR
    kw = dict(q=s['q'][None], c=np.array([[s['c']]]))
    if umax is not None:
        kw.update(D=np.array([[[0.0, 1.0]]]), d=np.array([[umax]]))
    return np.array([[[s['a']]]]), np.array([[[s['b']]]]), s['H'][None], 1, kw


def case_scalar_free():
    """nx = nu = p = N = 1 without rows: stage 0 is also the last stage."""
    return _case('scalar_free', lambda: _scalar(None))


def case_scalar_bound():
    """The same with u <= umax active (umax 0.3 below the free optimum)."""
    s = SCALAR
    return _case('scalar_bound', lambda: _scalar(scalar_closed_form(s['a'], s['b'], s['c'], s['H'], s['q'])[1] - 0.3))


def case_unstable():
    """nx 2 / nu 1 / p 2 with rho(A_1 A_0) > 1 and the input box at 0.7 of the free orbit's largest input."""
    def make():
        A, B, H, q, c = _model(31, 2, 1, 2)
        A = A * np.sqrt(1.5 / max(abs(np.linalg.eigvals(A[1] @ A[0]))))
        assert max(abs(np.linalg.eigvals(A[1] @ A[0]))) > 1.0
        return A, B, H, 1, _box(A, B, H, q, c, 0.7)
    return _case('unstable', make)


def case_eig_one():
    """nx 2 / nu 1 / p 1, the double integrator: A has the eigenvalue 1 twice, (A, B) is controllable; one bound on u... none is needed: u = -c_2."""
    def make():
        A = np.array([[[1.0, 1.0], [0.0, 1.0]]]); B = np.array([[[0.5], [1.0]]])
        H = np.array([[[2.0, 0.2, 0.1], [0.2, 1.0, 0.0], [0.1, 0.0, 0.5]]])
        kw = dict(q=np.array([[0.7, -0.4, 0.2]]), c=np.array([[0.3, -0.2]]), D=np.array([[[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]]), d=np.array([[-0.6, 2.0]]))
        return A, B, H, 1, kw
    return _case('eig_one', make)


RAGGED_ROWS, RAGGED_EROWS = [0, 4, 1], [1, 0, 0]


def _ragged():
    A, B, H, q, c = _model(33, 3, 2, 3)
    return A, B, H, 1, _rows(34, A, B, H, q, c, RAGGED_ROWS, RAGGED_EROWS)


def case_ragged():
    """nx 3 / nu 2 / p 3, inequality rows 0 / 4 / 1 (nd = 4), equality rows 1 / 0 / 0."""
    return _case('ragged', _ragged)


def case_wide_rows():
    """nx 2 / nu 1 / p 2 with nd = 7 > n + 1 rows at phase 0 and 3 at phase 1."""
    def make():
        A, B, H, q, c = _model(35, 2, 1, 2)
        return A, B, H, 1, _rows(36, A, B, H, q, c, [7, 3], [0, 0], every=4)
    return _case('wide_rows', make)


def case_odd():
    """nx 5 / nu 3 / p 4: odd sizes, rows 3 / 2 / 0 / 3, equality rows 0 / 1 / 0 / 2."""
    def make():
        A, B, H, q, c = _model(37, 5, 3, 4)
        return A, B, H, 1, _rows(38, A, B, H, q, c, [3, 2, 0, 3], [0, 1, 0, 2])
    return _case('odd', make)


def case_two_periods():
    """ragged over two periods: the one-period answer twice."""
    def make():
        c = case_ragged()
        return c['A'], c['B'], c['H'], 2, c['kw']
    return _case('two_periods', make)


def roll_kw(kw, shift=1):
    return {k: (None if x is None else np.roll(x, shift, axis=0)) for k, x in kw.items()}


def case_rolled():
    """ragged with every stage array rolled by one stage: the answer rolled by one stage."""
    def make():
        c = case_ragged()
        return np.roll(c['A'], 1, axis=0), np.roll(c['B'], 1, axis=0), np.roll(c['H'], 1, axis=0), 1, roll_kw(c['kw'])
    return _case('rolled', make)


def case_stage_shape():
    """nx 24 / nu 8 / p 6 with the 16-row input box at half the free orbit's largest input: the stage shape of scripts/mpc_qp_gain_timing.py."""
    def make():
        A, B, H, q, c = _model(39, 24, 8, 6)
        return A, B, H, 1, _box(A, B, H, q, c, 0.5)
    return _case('stage_shape', make)


def case_no_orbit():
    """A = I, B = 0, c != 0: no periodic trajectory."""
    def make():
        H = np.eye(3)[None]
        return np.eye(2)[None], np.zeros((1, 2, 1)), H, 1, dict(c=np.array([[0.3, -0.1]]))
    return _case('no_orbit', make)


def case_not_convex():
    """ragged with H_uu = -50 I at phase 1."""
    def make():
        c = case_ragged()
        H = c['H'].copy(); H[1, 3:, 3:] = -50.0 * np.eye(2)
        return c['A'], c['B'], H, 1, c['kw']
    return _case('not_convex', make)


FEASIBLE = [case_scalar_free, case_scalar_bound, case_unstable, case_eig_one, case_ragged, case_wide_rows, case_odd, case_two_periods, case_rolled,
            case_stage_shape]
FAILING = [(case_no_orbit, (1, 2, 3)), (case_not_convex, (2,))]      # (case, the statuses it may end with)


def solve_case(c):
    """A case through (a) and (b), once per process."""
    key = ('solved', c['name'])
    if key not in _CACHE:
        _CACHE[key] = solve(c['A'], c['B'], c['H'], c['periods'], **c['kw'])
    return _CACHE[key]


def batch_of(c):
    """A case -> the arguments of periodic_qp_batch with one member: dict A, B, H, q, offset, D, d, ndcnt, J, r, necnt, periods."""
    kw = c['kw']
    one = lambda k: None if kw.get(k) is None else np.ascontiguousarray(kw[k][None], float)
    cnt = lambda k: None if kw.get(k) is None else np.ascontiguousarray(np.asarray(kw[k])[None], np.int32)
    return dict(A=c['A'][None].copy(), B=c['B'][None].copy(), H=c['H'][None].copy(), q=one('q'), offset=one('c'), D=one('D'), d=one('d'), ndcnt=cnt('rows'),
                J=one('J'), r=one('r'), necnt=cnt('erows'), periods=c['periods'])


def many(nb=520, seed=41):
    """`scalar` with distinct data and the bound u <= umax, active on every other member -> batch arguments and the closed forms x, u, active [nb]."""
    if 'many' not in _CACHE:
        rng = np.random.default_rng(seed)
        a = rng.uniform(-0.8, 0.8, nb); b = rng.uniform(0.5, 1.5, nb) * rng.choice([-1.0, 1.0], nb); c = rng.uniform(-1.0, 1.0, nb)
        H = np.zeros((nb, 1, 2, 2)); H[:, 0, 0, 0] = rng.uniform(1.0, 3.0, nb); H[:, 0, 1, 1] = rng.uniform(1.0, 3.0, nb)
        H[:, 0, 0, 1] = H[:, 0, 1, 0] = rng.uniform(-0.5, 0.5, nb)
        q = rng.uniform(-2.0, 2.0, (nb, 1, 2))
        D = np.zeros((nb, 1, 1, 2)); D[..., 1] = 1.0
        d = np.zeros((nb, 1, 1)); x = np.zeros(nb); u = np.zeros(nb); act = np.zeros(nb, bool)
        for i in range(nb):
            uf = scalar_closed_form(a[i], b[i], c[i], H[i, 0], q[i, 0])[1]
            d[i, 0, 0] = uf + (-0.3 if i % 2 == 0 else 0.4)
            x[i], u[i], act[i] = scalar_closed_form(a[i], b[i], c[i], H[i, 0], q[i, 0], d[i, 0, 0])
        _CACHE['many'] = (dict(A=a.reshape(nb, 1, 1, 1), B=b.reshape(nb, 1, 1, 1), H=H, q=q, offset=c.reshape(nb, 1, 1), D=D, d=d), x, u, act)
    return _CACHE['many']
