"""Plain-numpy statement of the MPC step with EQUALITY rows and a TERMINAL constraint (the reference's pmpc.py: g(x, u) = 0 at every stage and
p_operator(x_N - x_ref) = 0 at the end).  Test infrastructure of test_mpc_qp_eq_cpu.py / test_gpu_mpc_qp_eq.py on top of mpc_qp_reference and
mpc_qp_soft_reference (imported, not changed).  To the QP of those two it adds, with k_j = (k0 + j) mod p and k_N = (k0 + N) mod p,

    J_k z_j = r_k  (first erows_k rows of stage k),  j = 0 .. N-1,        Tx_{k_N} x_N = 0  (nt rows; terminal='constraint' is Tx = I).

`dense_eq` adds them to the dense problem of mpc_qp_reference.dense as  Je v = re  (the stage rows, then the terminal rows).

Method (a), `ipm_eq`: the eliminated iteration of mpc_qp_soft_reference.ipm_soft (the hard one when no row is soft) where an equality row is a hard row
WITHOUT a slack.  The library runs the same iteration stage by stage (csrc/tmpc_mpc_qp.h, the EQ instantiations); the rules, stated here and mirrored there:
    multiplier nu of a row: free sign, starts at 0, no step-length limit, no part in mu, sigma or the corrector;
    weight     the constant 1 / RHO (what an inequality row may reach): the Newton system gets Je' (1 / RHO) Je and the right-hand side
               Je' (nu + (1 / RHO)(Je v - re)); then dnu = (1 / RHO)(Je dv + Je v - re).  The error of the regularisation in the row equation is RHO dnu and
               vanishes with the step; the residual Je v - re is taken from the iterate;
    stop       r_p also takes max_i |J z - r|_i / max(1, |r_i|) and max|Tx x_N| / max(1, max|x|); the scale of r_d takes J' nu of the stage rows; max lam stays
               over lam alone.
An instance whose rows cannot be met (N nu too short to reach Tx x_N = 0, or a row of stage 0 on x_0 alone that x_0 violates) ends with status 1.
Method (b), `polish_eq`: truth.  The states of (a) as in polish_soft, the rows of Je as equalities, one dense KKT solve; the certificate is that of polish_soft
and the stacked equality and active rows having full row rank (`rank_ok`: the multipliers are defined).  With dependent rows the system is solved in the
least-squares sense: the solution is defined, the multipliers are not (certificate False, `sol_ok` tells the rest of the certificate).

The cases are those of mpc_qp_reference with rows of this module; X0 is scaled per case so that every instance is feasible with margin >= MARGIN_MIN."""
import numpy as np

import lqr_horizon_reference as lh
import mpc_qp_reference as mq
import mpc_qp_soft_reference as sq

# (a) against (b) over every case below, relative to max(1, max|.|) of (b) (solution) and max(1, max lam, max|nu|) of (b) (multipliers).  Measured
# (test_mpc_qp_eq_cpu.py prints every figure and asserts the bound); rounded up to one digit.
EQ_IPM_VS_POLISH = 4e-10
# (b) against u_0 = -K_0 x_0 of lqr_horizon_reference.horizon_lqr(terminal='constraint') without inequality rows (test_mpc_qp_eq_cpu.py), rounded up likewise.
EQ_POLISH_VS_LQR = 2e-11
MARGIN_MIN = sq.MARGIN_MIN


def dense_eq(A, B, H, N, k0, x0, J=None, r=None, erows=None, Tx=None, **kw):
    """mpc_qp_reference.dense plus Je [me, nv], re, escale (max(1, |r_i|) of a stage row, 0 marks a terminal row), estage / erow (of each stage row), ne, nt.
    J [p,ne,n], r [p,ne] (None: zero), erows [p] (None: all ne), Tx [p,nt,nx] or 'constraint' (the identity)."""
    P = mq.dense(A, B, H, N, k0, x0, **kw)
    p, nx, mb = A.shape[0], P['nx'], P['mb']
    nv = len(P['c'])
    ne = 0 if J is None else J.shape[1]
    if erows is None:
        erows = np.full(p, ne)
    Je, re, es, st, rw = [], [], [], [], []
    for j in range(N):
        k = (k0 + j) % p
        for i in range(int(erows[k])):
            g = np.zeros(nv)
            g[P['iu'](j)] = J[k, i, nx:]
            ri = 0.0 if r is None else r[k, i]
            rhs = ri
            if j == 0:
                rhs = ri - J[k, i, :nx] @ x0
            else:
                g[P['ix'](j)] = J[k, i, :nx]
            Je.append(g); re.append(rhs); es.append(max(1.0, abs(ri))); st.append(j); rw.append(i)
    nt = 0
    if Tx is not None:
        T = np.eye(nx) if isinstance(Tx, str) else np.asarray(Tx[(k0 + N) % p], float)
        nt = T.shape[0]
        for i in range(nt):
            g = np.zeros(nv)
            g[P['ix'](N)] = T[i]
            Je.append(g); re.append(0.0); es.append(0.0)
    P.update(Je=np.array(Je).reshape(len(Je), nv), re=np.array(re), escale=np.array(es), estage=np.array(st, int), erow=np.array(rw, int), ne=ne, nt=nt)
    return P


def unpack_nu(P, nu):
    """The multipliers of the rows of Je -> Nu [N, ne], NuT [nt]."""
    Nu = np.zeros((P['N'], P['ne']))
    ms = len(P['estage'])
    if ms:
        Nu[P['estage'], P['erow']] = nu[:ms]
    return Nu, np.array(nu[ms:], float)


def ipm_eq(P, cvec=None, tol=mq.TOL, max_iter=mq.MAX_ITER, augmented=False):
    """Method (a) -> dict v, lam, s, e, nu (of e >= 0), nue (of the rows of Je), iters, status, mu, rp, rd.  cvec: one weight per row of G (None: all hard).
    augmented: the same Newton system with dnue as an unknown, its rows [Je, -RHO I] kept as rows: no 1 / RHO stands in the matrix, and dnue is not formed as
    the difference Je dv + req blown up by 1 / RHO (the truth path of tests/qp_path_reference.py); the iteration and its rules are the same."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, m, ne = len(c), len(h), len(b)
    Nmb = P['N'] * P['mb']
    RHO = mq.RHO
    if cvec is None:
        cvec = np.full(m, np.inf)
    soft = np.isfinite(cvec)
    ms = int(soft.sum())
    term = P['escale'] == 0.0
    Js = np.where(term[:, None], 0.0, Je)
    Cx = Cm[:, Nmb:]
    Zn = np.concatenate([np.eye(Nmb), -np.linalg.solve(Cx, Cm[:, :Nmb])])
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0) if m else np.zeros(0)
    lam = np.where(soft, 0.5 * np.where(soft, cvec, 0.0), 1.0); nu = np.where(soft, lam, 1.0)
    e = np.where(soft, s, 0.0)
    nue = np.zeros(len(re))
    xs0 = np.abs(P['x0']).max()
    status, it = 1, 0
    mu = rp = rd = np.nan
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            gs = Q @ v + c + G.T @ lam + Js.T @ nue
            g = gs + (Je - Js).T @ nue
            pi = np.linalg.solve(Cx.T, -g[Nmb:])
            rdv = g + Cm.T @ pi
            rpe = Cm @ v - b; rpi = G @ v - e + s - h; req = Je @ v - re
            mu = (float(lam @ s) + float(e[soft] @ nu[soft])) / (m + ms) if m else 0.0
            xsc = max(1.0, xs0, np.abs(v[Nmb:]).max())
            rp = max(np.abs(rpi / P['dscale']).max() if m else 0.0, np.abs(rpe).max() / xsc, np.abs(req / np.where(term, xsc, P['escale'])).max() if len(re) else 0.0)
            rd = np.abs(rdv[:Nmb]).max() / max(1.0, np.abs(gs).max())
            lmax = lam.max() if m else 0.0
            if not np.isfinite([mu, rp, rd, lmax]).all():
                status = 3; break
            if rp <= tol and rd <= tol and mu <= mq.MU_FACTOR * tol * max(1.0, lmax):
                status = 0; break
            if it == max_iter:
                break
            w = np.where(soft, 1.0 / (s / lam + e / nu + RHO), lam / (s + RHO * lam))
            Kmat = np.block([[Q + G.T @ (w[:, None] * G) + Je.T @ Je / RHO, Cm.T], [Cm, np.zeros((ne, ne))]])
            if not np.isfinite(Kmat).all():
                status = 3; break
            red = Zn.T @ Kmat[:nv, :nv] @ Zn
            if np.linalg.eigvalsh(red).min() <= 0:
                status = 2; break
            me = len(re)
            if augmented:
                Kaug = np.block([[Q + G.T @ (w[:, None] * G), Cm.T, Je.T], [Cm, np.zeros((ne, ne + me))], [Je, np.zeros((me, ne)), -RHO * np.eye(me)]])

            def solve(c1, c2):
                beta = rpi - s + e + c1 / lam - np.where(soft, c2 / nu, 0.0)
                if augmented:
                    sol = np.linalg.solve(Kaug, np.concatenate([-(rdv + G.T @ (w * beta)), -rpe, -req]))
                    dv, dn = sol[:nv], sol[nv + ne:]
                else:
                    dv = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta) + Je.T @ (req / RHO)), -rpe]))[:nv]
                    dn = (Je @ dv + req) / RHO
                dl = w * (beta + G @ dv)
                de = np.where(soft, -e + c2 / nu + (e / nu) * dl, 0.0)
                return dv, dl, -rpi - G @ dv + de + RHO * dl, de, dn

            def length(dl, ds, de):
                a = 1e300
                for x, dx in ((s, ds), (lam, dl), (e[soft], de[soft]), (nu[soft], -dl[soft])):
                    neg = dx < 0
                    if neg.any():
                        a = min(a, (-x[neg] / dx[neg]).min())
                return a
            z0 = np.zeros(m)
            dv, dl, ds, de, dn = solve(z0, z0)
            if m:
                aa = min(1.0, length(dl, ds, de))
                mu_aff = (float((lam + aa * dl) @ (s + aa * ds)) + float((e + aa * de)[soft] @ (nu - aa * dl)[soft])) / (m + ms)
                sigmu = (mu_aff / mu) ** 3 * mu
                dv, dl, ds, de, dn = solve(sigmu - ds * dl, sigmu + de * dl)
            al = min(1.0, mq.STEP_BACK * length(dl, ds, de))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; e = e + al * de; nu = nu - al * dl; nue = nue + al * dn
    return dict(v=v, lam=lam, s=s, e=e, nu=np.where(soft, nu, 0.0), nue=nue, iters=it, status=status, mu=mu, rp=rp, rd=rd)


def polish_eq(P, cvec, state):
    """Method (b) -> dict v, lam, e, nue, slack, eqres (max|Je v - re|), stat, margin, rank_ok, sol_ok (the certificate but the rank), certificate, nact, nviol,
    state."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, ne, mq_ = len(c), len(b), len(re)
    if cvec is None:
        cvec = np.full(len(h), np.inf)
    state = np.array(state)
    fixed = ~G.any(axis=1) if len(h) else np.zeros(0, bool)
    state[fixed] = np.where(np.isfinite(cvec[fixed]) & (h[fixed] < 0), sq.VIOLATED, sq.INACTIVE)
    act, vio = (state == sq.ACTIVE) & ~fixed, (state == sq.VIOLATED) & ~fixed
    if ((state == sq.VIOLATED) & ~np.isfinite(cvec)).any():
        raise ValueError('polish_eq: a hard row cannot be violated')
    Ga, Gv = G[act], G[vio]
    na, nvio = Ga.shape[0], Gv.shape[0]
    o1, o2, o3 = nv + ne, nv + ne + mq_, nv + ne + mq_ + na
    nt = o3 + nvio
    K = np.zeros((nt, nt))
    K[:nv, :nv] = Q; K[:nv, nv:o1] = Cm.T; K[nv:o1, :nv] = Cm
    K[:nv, o1:o2] = Je.T; K[o1:o2, :nv] = Je
    K[:nv, o2:o3] = Ga.T; K[o2:o3, :nv] = Ga
    rr = slice(o3, nt)
    K[rr, :nv] = Gv; K[rr, rr] = -np.eye(nvio)
    rhs = np.concatenate([-c - Gv.T @ cvec[vio], b, re, h[act], h[vio]])
    rows = np.zeros((nt - nv, nv + nvio)); rows[:, :nv] = K[nv:, :nv]; rows[o3 - nv:, nv:] = -np.eye(nvio)
    rank_ok = bool(np.linalg.matrix_rank(rows) == rows.shape[0])
    sol = np.linalg.solve(K, rhs) if rank_ok else np.linalg.lstsq(K, rhs, rcond=None)[0]
    v, pi, nue = sol[:nv], sol[nv:o1], sol[o1:o2]
    lam = np.zeros(len(h)); lam[act] = sol[o2:o3]; lam[vio] = cvec[vio]
    e = np.zeros(len(h)); e[vio] = sol[rr]
    fv = fixed & (state == sq.VIOLATED)
    lam[fv] = cvec[fv]; e[fv] = -h[fv]; vio = vio | fv
    slack = h - G @ v + e
    grad = Q @ v + c
    stat = np.abs(grad + Cm.T @ pi + G.T @ lam + Je.T @ nue).max() / max(1.0, np.abs(grad).max())
    eqres = max(np.abs(Je @ v - re).max() if mq_ else 0.0, np.abs(Cm @ v - b).max())
    strict = [slack[state == sq.INACTIVE], lam[act], (cvec - lam)[act], e[vio]]
    margin = min([x.min() for x in strict if x.size] + [np.inf])
    sol_ok = bool(margin > 0 and stat <= 1e-11 and eqres <= 1e-11 * max(1.0, np.abs(v).max()))
    return dict(v=v, lam=lam, e=e, nue=nue, slack=slack, eqres=eqres, stat=stat, margin=margin, rank_ok=rank_ok, sol_ok=sol_ok, certificate=sol_ok and rank_ok,
                nact=int(na + vio.sum()), nviol=int(vio.sum()), state=state)


def feasible(P):
    """Whether the rows of the dense problem with every row hard (dynamics, Je, G) have a common point: the equalities by least squares, then, in their null
    space v = v0 + Z y, the LP  min t  s.t.  G Z y - t <= h - G v0, t >= -1  (scipy.optimize.linprog): feasible when t <= 0 to rounding.  Used only to tell
    which instances the cases may contain."""
    Cm, b, G, h, Je, re = (P[k] for k in ('Cm', 'b', 'G', 'h', 'Je', 're'))
    Aeq = np.vstack([Cm, Je]); beq = np.concatenate([b, re])
    v = np.linalg.lstsq(Aeq, beq, rcond=None)[0]
    if np.abs(Aeq @ v - beq).max() > 1e-9 * max(1.0, np.abs(beq).max()):
        return False
    if not len(h):
        return True
    from scipy.optimize import linprog
    _, sv, Vt = np.linalg.svd(Aeq)
    rank = int((sv > 1e-10 * sv[0]).sum())
    Z = Vt[rank:].T
    ny = Z.shape[1]
    res = linprog(np.concatenate([np.zeros(ny), [1.0]]), A_ub=np.hstack([G @ Z, -np.ones((len(h), 1))]), b_ub=h - G @ v, bounds=[(None, None)] * ny + [(-1.0, None)])
    return bool(res.status == 0 and res.x[-1] <= 1e-9)


def solve_eq(A, B, H, N, k0, x0, penalty=None, tol=mq.TOL, max_iter=mq.MAX_ITER, **kw):
    """(a) then (b) on one instance (kw: q, Pf, D, d, rows, J, r, erows, Tx; penalty [p, nd] or None) -> dict a, b, X, U, Lam, Eps, Nu, NuT of (b), Xa, Ua, Lama,
    Epsa, Nua, NuTa of (a), nact0, nviol0, eres0 (max|J z_0 - r| of (b) at stage 0), P, cvec."""
    P = dense_eq(A, B, H, N, k0, x0, **kw)
    cvec = sq.row_penalty(P, penalty, k0) if penalty is not None else np.full(len(P['h']), np.inf)
    a = ipm_eq(P, cvec, tol, max_iter)
    bb = polish_eq(P, cvec, sq.states_of(a, cvec) if len(P['h']) else np.zeros(0, int))
    st = bb['state']
    X, U, Lam = mq.unpack(P, bb['v'], bb['lam'])
    Xa, Ua, Lama = mq.unpack(P, a['v'], a['lam'])
    Nu, NuT = unpack_nu(P, bb['nue']); Nua, NuTa = unpack_nu(P, a['nue'])
    s0 = P['stage'] == 0
    return dict(a=a, b=bb, X=X, U=U, Lam=Lam, Eps=mq.unpack(P, bb['v'], bb['e'])[2], Nu=Nu, NuT=NuT, Xa=Xa, Ua=Ua, Lama=Lama, Epsa=mq.unpack(P, a['v'], a['e'])[2],
                Nua=Nua, NuTa=NuTa, nact0=int((s0 & (st != sq.INACTIVE)).sum()) if len(st) else 0, nviol0=int((s0 & (st == sq.VIOLATED)).sum()) if len(st) else 0,
                eres0=stage_eres(A, k0, X[0], U[0], kw.get('J'), kw.get('r'), kw.get('erows')), P=P, cvec=cvec)


def stage_eres(A, k, x, u, J, r, erows):
    """max|J_k [x; u] - r_k| over the rows of stage k; 0 at a stage without rows."""
    if J is None:
        return 0.0
    rk = int(J.shape[1] if erows is None else erows[k])
    if not rk:
        return 0.0
    return float(np.abs(J[k, :rk] @ np.concatenate([x, u]) - (0.0 if r is None else r[k, :rk])).max())


def ab_disagreement(r):
    """(a) against (b): the solution relative to max(1, max|.|) of (b); lam, e, nu relative to max(1, max lam, max|nu|) of (b)."""
    rel = lambda x, y, sc: np.abs(x - y).max() / sc if y.size else 0.0
    ls = max([1.0] + [np.abs(r[k]).max() for k in ('Lam', 'Nu', 'NuT') if r[k].size])
    return dict(sol=max(rel(r['Xa'], r['X'], max(1.0, np.abs(r['X']).max())), rel(r['Ua'], r['U'], max(1.0, np.abs(r['U']).max()))),
                lam=rel(r['Lama'], r['Lam'], ls), e=rel(r['Epsa'], r['Eps'], ls), nu=max(rel(r['Nua'], r['Nu'], ls), rel(r['NuTa'], r['NuT'], ls)))


def mult_scale(r):
    return max([1.0] + [np.abs(r[k]).max() for k in ('Lam', 'Nu', 'NuT') if r[k].size])


def closed_loop_eq(A, B, H, N, k0, x0, T, penalty=None, **kw):
    """The receding-horizon loop on (b) -> dict X, U, nact, nviol [T] (stage 0), hres [T] (-inf at a stage without rows), eres [T], margin, certificate."""
    p = A.shape[0]
    D, d, rows = kw.get('D'), kw.get('d'), kw.get('rows')
    X = [np.asarray(x0, float)]; U = []; nact = []; nviol = []; hres = []; eres = []; margin = np.inf; cert = True
    for t in range(T):
        k = (k0 + t) % p
        r = solve_eq(A, B, H, N, k, X[-1], penalty, **kw)
        u = r['U'][0]
        z = np.concatenate([X[-1], u])
        rk = 0 if D is None else int(D.shape[1] if rows is None else rows[k])
        hres.append((D[k, :rk] @ z - d[k, :rk]).max() if rk else -np.inf)
        eres.append(r['eres0'])
        U.append(u); nact.append(r['nact0']); nviol.append(r['nviol0']); margin = min(margin, r['b']['margin'])
        cert = cert and r['b']['certificate'] and r['a']['status'] == 0
        X.append(A[k] @ X[-1] + B[k] @ u)
    return dict(X=np.array(X), U=np.array(U), nact=np.array(nact), nviol=np.array(nviol), hres=np.array(hres), eres=np.array(eres), margin=margin, certificate=cert)


def kkt_check_eq(A, B, H, N, k0, X, U, Lam, Nu, NuT, Eps=None, penalty=None, q=None, Pf=None, D=None, d=None, rows=None, J=None, r=None, erows=None, Tx=None):
    """Solver-independent figures of a returned open-loop solution: dyn (dynamics residual / max(1, max|X|)), eq (max|J z - r| / max(1, |r|)), term
    (max|Tx x_N| / max(1, max|X|)), viol (max(D z - e - d) / max(1, |d|); -inf without rows), lam_min, comp (max|lam (d - D z + e)| / max(1, max lam)),
    comp_e (max|e (c - lam)| over the soft rows, same scale), stat (the u rows of the stationarity condition with the adjoint
    pi_j = (H z_j + q + D' lam_j + J' nu_j)_x + A' pi_{j+1}, pi_N = Pf x_N + Tx' nu_T, relative to max(1, max|H z + q + D' lam + J' nu|))."""
    p, nx = A.shape[0], A.shape[1]
    kN = (k0 + N) % p
    dyn = eq = comp = comp_e = stat = gmax = 0.0
    viol, lam_min = -np.inf, np.inf
    xs = max(1.0, np.abs(X).max())
    pi = np.zeros(nx) if Pf is None else ((Pf[kN] + Pf[kN].T) / 2) @ X[N]
    term = 0.0
    if Tx is not None:
        T = np.eye(nx) if isinstance(Tx, str) else np.asarray(Tx[kN], float)
        pi = pi + T.T @ NuT
        term = np.abs(T @ X[N]).max() / xs
    for j in range(N - 1, -1, -1):
        k = (k0 + j) % p
        z = np.concatenate([X[j], U[j]])
        E = np.concatenate([A[k], B[k]], axis=1)
        dyn = max(dyn, np.abs(E @ z - X[j + 1]).max())
        g = ((H[k] + H[k].T) / 2) @ z + (0 if q is None else q[k])
        rk = 0 if D is None else int(D.shape[1] if rows is None else rows[k])
        if rk:
            lam = Lam[j, :rk]
            e = np.zeros(rk) if Eps is None else Eps[j, :rk]
            g = g + D[k, :rk].T @ lam
            res = D[k, :rk] @ z - e - d[k, :rk]
            viol = max(viol, (res / np.maximum(1.0, np.abs(d[k, :rk]))).max())
            comp = max(comp, np.abs(lam * res).max()); lam_min = min(lam_min, lam.min(), e.min())
            if penalty is not None:
                sf = np.isfinite(penalty[k, :rk])
                if sf.any():
                    comp_e = max(comp_e, np.abs(e[sf] * (penalty[k, :rk] - lam)[sf]).max()); lam_min = min(lam_min, (penalty[k, :rk] - lam)[sf].min())
        ek = 0 if J is None else int(J.shape[1] if erows is None else erows[k])
        if ek:
            rv = np.zeros(ek) if r is None else r[k, :ek]
            g = g + J[k, :ek].T @ Nu[j, :ek]
            eq = max(eq, (np.abs(J[k, :ek] @ z - rv) / np.maximum(1.0, np.abs(rv))).max())
        gmax = max(gmax, np.abs(g).max())
        full = g + E.T @ pi
        stat = max(stat, np.abs(full[nx:]).max())
        pi = full[:nx]
    lmax = max(1.0, np.abs(Lam).max()) if Lam is not None and Lam.size else 1.0
    return dict(dyn=dyn / xs, eq=eq, term=term, viol=viol, lam_min=lam_min, comp=comp / lmax, comp_e=comp_e / lmax, stat=stat / max(1.0, gmax))


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def _case(name, base, scale, J=None, r=None, erows=None, Tx=None, penalty_f=None, no_rows=False, lqr_J=None):
    """base: a case dict of mpc_qp_reference.  Returns dict A, B, H, Pf, X0 (scaled), N, k0, q, D, d, rows, ncnt, J, r, erows, Tx ('constraint', an array
    [nb,p,nt,nx] or None), penalty [nb,p,nd] or None."""
    if name not in _CACHE:
        c = dict(base)
        c['X0'] = scale * base['X0']
        if no_rows:
            c.update(D=None, d=None, rows=None, ncnt=None)
        c.update(J=J, r=r, erows=erows, Tx=Tx, penalty=None, name=name)
        if penalty_f is not None:
            hard = [[solve_eq(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, **kwargs(c, b)) for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]
            lmax = max(h['Lam'].max() for hb in hard for h in hb)
            c['penalty'] = np.full(c['d'].shape, penalty_f * (lmax if lmax > 0 else 1.0))
        _CACHE[name] = c
    return _CACHE[name]


def kwargs(c, b=0):
    """The keyword arguments of dense_eq / solve_eq / closed_loop_eq for member b of a case."""
    pick = lambda k: None if c[k] is None else c[k][b]
    tx = c['Tx'] if c['Tx'] is None or isinstance(c['Tx'], str) else c['Tx'][b]
    return dict(q=pick('q'), Pf=c['Pf'][b], D=pick('D'), d=pick('d'), rows=pick('rows'), J=pick('J'), r=pick('r'), erows=pick('erows'), Tx=tx)


def _rows(seed, nb, p, n, counts, rscale):
    rng = np.random.default_rng(seed)
    ne = max(counts)
    J = np.zeros((nb, p, ne, n)); r = np.zeros((nb, p, ne))
    for k in range(p):
        J[:, k, :counts[k]] = rng.standard_normal((nb, counts[k], n)); r[:, k, :counts[k]] = rscale * rng.standard_normal((nb, counts[k]))
    return J, r, np.tile(np.asarray(counts), (nb, 1))


def _tx(seed, nb, p, nt, nx):
    return np.random.default_rng(seed).standard_normal((nb, p, nt, nx))


def case_term_box_nu1():
    """x_N = 0 on p 3 / nx 3 / nu 1, N = 5 from phase 2, the input box."""
    return _case('term_box_nu1', mq.case_box_nu1(), 0.8, Tx='constraint')


def case_term_box_nu2():
    """x_N = 0 on p 3 / nx 3 / nu 2, N = 4, the input box."""
    return _case('term_box_nu2', mq.case_box_nu2(), 1.0, Tx='constraint')


def case_term_p1():
    """x_N = 0 on p 1 / nx 3 / nu 2, N = 3, the input box."""
    return _case('term_p1', mq.case_single_phase(), 1.0, Tx='constraint')


def case_term_box_bench():
    """x_N = 0 on the bench stage shape nx 24 / nu 8, N = 6, the 16-row box."""
    return _case('term_box_bench', mq.case_box_bench(), 1.0, Tx='constraint')


def case_tx_box_nu2():
    """A general Tx with nt = 2 < nx = 3 on box_nu2."""
    return _case('tx_box_nu2', mq.case_box_nu2(), 1.0, Tx=_tx(21, 1, 3, 2, 3))


def case_rows_mixed_small(N=4):
    """Ragged equality rows (1 / 0 / 1) with r != 0 and 2 terminal rows on mixed_small, N = 4 or N = 2 < p."""
    J, r, er = _rows(22, 1, 3, 5, [1, 0, 1], 0.1)
    return _case('rows_mixed_small_%d' % N, mq.case_mixed_small(N), 0.3, J=J, r=r, erows=er, Tx=_tx(23, 1, 3, 2, 3))


def case_rows_mixed_small_N2():
    return case_rows_mixed_small(2)


def case_rows_mixed_bench():
    """mixed_bench with 2 rows per stage and 5 terminal rows."""
    J, r, er = _rows(24, 1, 2, 32, [2, 2], 0.1)
    return _case('rows_mixed_bench', mq.case_mixed_bench(), 0.3, J=J, r=r, erows=er, Tx=_tx(25, 1, 2, 5, 24))


def case_edge():
    """nx 40 / nu 24 at N = 2 with 2 rows per stage and Tx of 3 rows: the layout edge."""
    J, r, er = _rows(26, 1, 2, 64, [2, 1], 0.1)
    return _case('edge_eq', mq.case_layout_edge(), 0.3, J=J, r=r, erows=er, Tx=_tx(27, 1, 2, 3, 40))


def case_soft():
    """penalty (0.3 max lam of the hard solutions: some rows violated) plus equality rows plus terminal='constraint' on box_nu2."""
    J, r, er = _rows(28, 1, 3, 5, [1, 0, 1], 0.05)
    return _case('soft_eq', mq.case_box_nu2(), 1.0, J=J, r=r, erows=er, Tx='constraint', penalty_f=0.3)


def case_dependent_row():
    """rows_mixed_small with the row of phase 0 stated twice: the solution is defined, the multipliers are not."""
    b = case_rows_mixed_small()
    J = np.concatenate([b['J'], np.zeros_like(b['J'])], axis=2); r = np.concatenate([b['r'], np.zeros_like(b['r'])], axis=2)
    J[:, 0, 1] = J[:, 0, 0]; r[:, 0, 1] = r[:, 0, 0]
    return _case('dependent', mq.case_mixed_small(4), 0.3, J=J, r=r, erows=np.array([[2, 0, 1]]), Tx=b['Tx'])


def case_lqr(which):
    """No inequality rows, homogeneous J of the lqr_horizon_reference case, terminal='constraint': the fixed-active-set law u_0 = -K_0 x_0."""
    base, lq = {'nu1': (mq.case_box_nu1, lh.case_no_rows), 'nu2': (mq.case_box_nu2, lh.case_ragged_rows), 'p1': (mq.case_single_phase, lh.case_single_phase),
                'bench': (mq.case_box_bench, lh.case_bench_stage_shape_ragged)}[which]
    l = lq()
    J = l['J']
    er = None if J is None else (np.tile(np.asarray(l['ncnt']), (J.shape[0], 1)) if l['ncnt'] is not None else np.full(J.shape[:2], J.shape[2]))
    return _case('lqr_' + which, base(), 1.0, J=J, erows=er, Tx='constraint', no_rows=True)


VALUE_CASES = [case_term_box_nu1, case_term_box_nu2, case_term_p1, case_term_box_bench, case_tx_box_nu2, case_rows_mixed_small, case_rows_mixed_small_N2,
               case_rows_mixed_bench, case_edge, case_soft]
SMALL = [case_term_box_nu1, case_rows_mixed_small, case_soft]
LQR_CASES = ['nu1', 'nu2', 'p1', 'bench']


def solve_case(c):
    """Every instance of a case through (a) and (b), once per process -> list [nb][ns] of the dicts of solve_eq."""
    key = ('solved', c['name'])
    if key not in _CACHE:
        _CACHE[key] = [[solve_eq(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, None if c['penalty'] is None else c['penalty'][b], **kwargs(c, b))
                        for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]
    return _CACHE[key]


def batch_of(c):
    """A case -> the batch arguments: dict A, B, H, X0, q, Pf, D, d, ndcnt, penalty, J, r, necnt, terminal, N, k0."""
    i32 = lambda x: None if x is None else np.ascontiguousarray(x, np.int32)
    return dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=i32(c['rows']), penalty=c['penalty'], J=c['J'], r=c['r'],
                necnt=i32(c['erows']), terminal=c['Tx'], N=c['N'], k0=c['k0'])


def infeasible_instances():
    """Three instances that no point satisfies, each as (A, B, H, N, k0, x0, kw): N nu = 2 < nt = nx = 3 (box_nu1 model at N = 2); a row of stage 0 on x_0
    alone that x_0 violates; input box plus x_N = 0 from a start too far away (box_nu1 at 8 times its X0)."""
    c = mq.case_box_nu1()
    A, B, H = c['A'][0], c['B'][0], c['H'][0]
    kw = dict(Pf=c['Pf'][0])
    out = [(A, B, H, 2, 2, c['X0'][0, 0], dict(kw, Tx='constraint'))]
    J = np.zeros((3, 1, 4)); J[:, 0, 0] = 1.0
    out.append((A, B, H, 5, 2, np.array([1.0, 0.2, -0.3]), dict(kw, J=J)))
    out.append((A, B, H, 5, 2, 8.0 * c['X0'][0, 0], dict(kw, D=c['D'][0], d=c['d'][0], rows=c['rows'][0], Tx='constraint')))
    return out
