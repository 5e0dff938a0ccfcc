"""Plain-numpy statement of the MPC step with QUADRATIC slack penalties (the reference's acados export carries them as ocp.cost.Zl / Zu next to zl / zu).
Test infrastructure of test_mpc_qp_quad_cpu.py / test_gpu_mpc_qp_quad.py on top of mpc_qp_reference and mpc_qp_soft_reference (imported, not changed).

`penalty` [p, nd] (the L1 weight c) and `penalty2` [p, nd] (the L2 weight Z >= 0) describe the rows of one problem:
    c = inf (Z = 0)    a hard row                                           D_i z <= d_i
    c > 0,  Z = 0      the soft row of mpc_qp_soft_reference                D_i z - e <= d_i, e >= 0, cost c e
    c > 0,  Z > 0      L1 + L2, two complementarity pairs                   D_i z - e <= d_i, e >= 0, cost c e + 1/2 Z e^2
    c = 0,  Z > 0      pure quadratic, ONE pair                             D_i z - e <= d_i, cost 1/2 Z e^2  (e = lam / Z >= 0 by itself)
On the dense problem of mpc_qp_reference.dense they become one pair of weights per row of G (`row_penalty` of the soft reference, once for each).

Method (a), `ipm_quad`: the iteration of mpc_qp_soft_reference.ipm_soft with these rules (csrc/tmpc_mpc_qp.h, the QUAD instantiations, mirrors them):
  L1 + L2 row   stationarity in e is c + Z e - lam - nu = 0.  Start s = max(d, 1), e = s, lam = nu = (c + Z e) / 2: both pairs carry the same product, and
                at Z = 0 this is the soft start.  dnu = Z de - dlam keeps stationarity at every iterate.  With nut = nu + Z e:
                w = 1 / (s / lam + e / nut + RHO),  beta = r_in - s + c1 / lam + (e nu - c2) / nut,  dlam = w (D dz + beta),
                de = (c2 - e nu + e dlam) / nut,  ds = -r_in - D dz + de + RHO dlam;  corrector c1 = sigma mu - ds_aff dlam_aff, c2 = sigma mu - de_aff dnu_aff;
                the step length runs over s, lam, e, nu; mu, sigma and the stop test as for a soft row.  A row with Z = 0 takes the soft row's statements.
  pure row      a hard row whose dual regularisation is exact instead of vanishing: r_in = D z - lam / Z + s - d,  w = lam / (s + (RHO + 1 / Z) lam),
                ds = -r_in - D dz + (RHO + 1 / Z) dlam,  start lam = 1, one pair in mu; the reported slack is e = lam / Z.
Method (b), `polish_quad`: truth.  One dense KKT solve with the violated two-pair rows carrying lam = c + Z e and the active pure rows carrying
G v - lam / Z = h; the certificate is that of polish_soft (every strict inequality holds, stationarity <= 1e-11), `margin` the smallest strict inequality.
Method (c), `lift_quad`: the slack as a pseudo-control with Z on its Hessian diagonal and c in q, the row -e <= 0 only on two-pair rows, through the EXISTING
hard iteration mpc_qp_reference.ipm.

nact counts lam > s; nviol counts the two-pair rows with e > nu and the pure rows with lam > s (on a pure row active means violated)."""
import numpy as np

import mpc_qp_reference as mq
import mpc_qp_soft_reference as ms

# (a) against (b) over every variant of VARIANTS and the three infeasible starts, the scales of mpc_qp_soft_reference.ab_disagreement but e relative to
# max(1, max e) of (b).  Measured (test_mpc_qp_quad_cpu.py prints every figure): over VARIANTS 1.7e-9 on the solution, 2.5e-9 on lam, 9.8e-11 on e (the smallest
# margin is 3.0e-4); over the infeasible starts 8.9e-9 on the solution (at Z = 5e5, where max lam = 4.5e5 loosens the threshold of mu), 1.4e-11 on lam,
# 1.2e-11 on e.  The worst of all, rounded up to one digit.
QUAD_IPM_VS_POLISH = 9e-9
MARGIN_MIN = ms.MARGIN_MIN
INACTIVE, ACTIVE, VIOLATED = ms.INACTIVE, ms.ACTIVE, ms.VIOLATED


def kinds(cvec, zvec):
    """-> (hard, two, pure, quad): c = inf; c > 0 finite (two pairs); c = 0 with Z > 0; two pairs with Z > 0."""
    hard = ~np.isfinite(cvec)
    pure = (cvec == 0) & (zvec > 0)
    two = ~hard & ~pure
    return hard, two, pure, two & (zvec > 0)


def ipm_quad(P, cvec, zvec, tol=mq.TOL, max_iter=mq.MAX_ITER):
    """Method (a) -> dict v, lam, s, e (lam / Z on pure rows), nu, iters, status (as ipm_soft), mu, rp, rd."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, m, ne = len(c), len(h), len(b)
    Nmb = P['N'] * P['mb']
    RHO = mq.RHO
    hard, two, pure, quad = kinds(cvec, zvec)
    mp = m + int(two.sum())
    zz = np.where(quad, zvec, 0.0)                                           # Z of the two-pair rows
    zinv = np.where(pure, 1.0 / np.where(pure, zvec, 1.0), 0.0)              # 1 / Z of the pure rows
    rz = RHO + zinv                                                          # the dual regularisation of a hard-like row: exact on a pure row
    Cx = Cm[:, Nmb:]
    Zn = np.concatenate([np.eye(Nmb), -np.linalg.solve(Cx, Cm[:, :Nmb])])
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0)
    e = np.where(two, s, 0.0)
    lam = np.where(two, 0.5 * (np.where(two, cvec, 0.0) + zz * e), 1.0); nu = np.where(two, lam, 1.0)     # (nu of a one-pair row is a placeholder: never read)
    xs0 = np.abs(P['x0']).max()
    status, it = 1, 0
    mu = rp = rd = np.nan
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            g = Q @ v + c + G.T @ lam
            pi = np.linalg.solve(Cx.T, -g[Nmb:])
            rdv = g + Cm.T @ pi
            rpe = Cm @ v - b; rpi = G @ v - np.where(pure, lam * zinv, e) + s - h
            mu = (float(lam @ s) + float(e[two] @ nu[two])) / mp if m else 0.0
            rp = max(np.abs(rpi / P['dscale']).max() if m else 0.0, np.abs(rpe).max() / max(1.0, xs0, np.abs(v[Nmb:]).max()))
            rd = np.abs(rdv[:Nmb]).max() / max(1.0, np.abs(g).max())
            lmax = lam.max() if m else 0.0
            if not np.isfinite([mu, rp, rd, lmax]).all():
                status = 3; break
            if rp <= tol and rd <= tol and mu <= mq.MU_FACTOR * tol * max(1.0, lmax):
                status = 0; break
            if it == max_iter:
                break
            nt = nu + zz * e                                                 # nu + Z e (nu itself at Z = 0)
            enu = np.where(quad, e * nu / nt, e)                             # e nu / nut (e itself at Z = 0: the soft row's statement)
            w = np.where(two, 1.0 / (s / lam + e / nt + RHO), lam / (s + rz * lam))
            Kmat = np.block([[Q + G.T @ (w[:, None] * G), Cm.T], [Cm, np.zeros((ne, ne))]])
            if not np.isfinite(Kmat).all():
                status = 3; break
            red = Zn.T @ Kmat[:nv, :nv] @ Zn
            if np.linalg.eigvalsh(red).min() <= 0:
                status = 2; break

            def solve(c1, c2):
                beta = rpi - s + enu + c1 / lam - np.where(two, c2 / nt, 0.0)
                dv = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta)), -rpe]))[:nv]
                dl = w * (beta + G @ dv)
                de = np.where(two, -enu + c2 / nt + (e / nt) * dl, 0.0)
                return dv, dl, -rpi - G @ dv + de + rz * dl, de, zz * de - dl

            def length(dl, ds, de, dn):
                a = 1e300
                for x, dx in ((s, ds), (lam, dl), (e[two], de[two]), (nu[two], dn[two])):
                    neg = dx < 0
                    if neg.any():
                        a = min(a, (-x[neg] / dx[neg]).min())
                return a
            z0 = np.zeros(m)
            dv, dl, ds, de, dn = solve(z0, z0)
            if m:
                aa = min(1.0, length(dl, ds, de, dn))
                mu_aff = (float((lam + aa * dl) @ (s + aa * ds)) + float((e + aa * de)[two] @ (nu + aa * dn)[two])) / mp
                sigmu = (mu_aff / mu) ** 3 * mu
                dv, dl, ds, de, dn = solve(sigmu - ds * dl, sigmu - de * dn)
            al = min(1.0, mq.STEP_BACK * length(dl, ds, de, dn))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; e = e + al * de; nu = nu + al * dn
    return dict(v=v, lam=lam, s=s, e=np.where(pure, lam * zinv, e), nu=np.where(two, nu, 0.0), iters=it, status=status, mu=mu, rp=rp, rd=rd)


def states_of(a, cvec, zvec):
    """The pattern of an iterate of (a): violated where a two-pair row has e > nu, else active where lam > s, else inactive."""
    _, two, _, _ = kinds(cvec, zvec)
    st = np.where(a['lam'] > a['s'], ACTIVE, INACTIVE)
    st[two & (a['e'] > a['nu'])] = VIOLATED
    return st


def polish_quad(P, cvec, zvec, state):
    """Method (b): hard and two-pair rows with state ACTIVE as equalities, two-pair rows with state VIOLATED as equalities with their slack free and
    lam = c + Z e, pure rows with state ACTIVE as G v - lam / Z = h -> dict v, lam, e (all rows; lam / Z on pure rows), slack = h - G v + e, certificate,
    margin, stat, nact, nviol, state.  A row on x_0 alone is a constant of the problem: its state follows from the sign of h."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, ne = len(c), len(b)
    hard, two, pure, _ = kinds(cvec, zvec)
    state = np.array(state)
    if ((state == VIOLATED) & ~two).any():
        raise ValueError('polish_quad: only a two-pair row can be in the state VIOLATED')
    fixed = ~G.any(axis=1)
    state[fixed] = np.where(two[fixed] & (h[fixed] < 0), VIOLATED, np.where(pure[fixed] & (h[fixed] < 0), ACTIVE, INACTIVE))
    act, vio, pac = (state == ACTIVE) & ~pure, state == VIOLATED, (state == ACTIVE) & pure
    Ga, Gv, Gp = G[act], G[vio], G[pac]
    na, nvio, npa = Ga.shape[0], Gv.shape[0], Gp.shape[0]
    o1, o2, o3 = nv + ne, nv + ne + na, nv + ne + na + nvio
    nt = o3 + npa
    K = np.zeros((nt, nt))
    K[:nv, :nv] = Q; K[:nv, nv:o1] = Cm.T; K[nv:o1, :nv] = Cm
    K[:nv, o1:o2] = Ga.T; K[o1:o2, :nv] = Ga
    K[:nv, o2:o3] = Gv.T * zvec[vio]; K[o2:o3, :nv] = Gv; K[o2:o3, o2:o3] = -np.eye(nvio)      # stationarity gets Gv' (c + Z e); the row is Gv v - e = h
    K[:nv, o3:] = Gp.T; K[o3:, :nv] = Gp; K[o3:, o3:] = -np.diag(1.0 / zvec[pac])              # the row is Gp v - lam / Z = h
    sol = np.linalg.solve(K, np.concatenate([-c - Gv.T @ cvec[vio], b, h[act], h[vio], h[pac]]))
    v, pi = sol[:nv], sol[nv:o1]
    lam = np.zeros(len(h)); e = np.zeros(len(h))
    lam[act] = sol[o1:o2]; e[vio] = sol[o2:o3]; lam[vio] = cvec[vio] + zvec[vio] * e[vio]
    lam[pac] = sol[o3:]; e[pac] = lam[pac] / zvec[pac]
    slack = h - G @ v + e
    grad = Q @ v + c
    stat = np.abs(grad + Cm.T @ pi + G.T @ lam).max() / max(1.0, np.abs(grad).max())
    strict = [slack[state == INACTIVE], lam[act], (cvec - lam)[act], e[vio], lam[pac]]         # (c - lam = inf on a hard row)
    margin = min([x.min() for x in strict if x.size] + [np.inf])
    return dict(v=v, lam=lam, e=e, slack=slack, stat=stat, margin=margin, certificate=bool(margin > 0 and stat <= 1e-11), nact=int(na + nvio + npa),
                nviol=int(nvio + npa), state=state)


def solve_quad(A, B, H, N, k0, x0, penalty, penalty2, tol=mq.TOL, max_iter=mq.MAX_ITER, dense=mq.dense, **kw):
    """(a) then (b) on one instance (penalty, penalty2 [p, nd]) -> the dict of mpc_qp_soft_reference.solve_soft (nviol0: the violated two-pair rows and the
    active pure rows of stage 0) with zvec.  `dense` builds the dense problem (mpc_qp_reference.dense)."""
    P = dense(A, B, H, N, k0, x0, **kw)
    cvec, zvec = ms.row_penalty(P, penalty, k0), ms.row_penalty(P, penalty2, k0)
    return finish_quad(P, cvec, zvec, ipm_quad(P, cvec, zvec, tol, max_iter))


def finish_quad(P, cvec, zvec, a, polish=polish_quad):
    st = states_of(a, cvec, zvec)
    bb = polish(P, cvec, zvec, st)
    st = bb['state']
    pure = kinds(cvec, zvec)[2] if len(cvec) else np.zeros(0, bool)
    X, U, Lam = mq.unpack(P, bb['v'], bb['lam'])
    Xa, Ua, Lama = mq.unpack(P, a['v'], a['lam'])
    s0 = P['stage'] == 0
    viol = (st == VIOLATED) | ((st == ACTIVE) & pure)
    return dict(a=a, b=bb, state=st, X=X, U=U, Lam=Lam, Eps=mq.unpack(P, bb['v'], bb['e'])[2], Xa=Xa, Ua=Ua, Lama=Lama, Epsa=mq.unpack(P, a['v'], a['e'])[2],
                State=mq.unpack(P, bb['v'], st.astype(float))[2].astype(int), nact0=int((s0 & (st != INACTIVE)).sum()), nviol0=int((s0 & viol).sum()),
                P=P, cvec=cvec, zvec=zvec)


def ab_disagreement(r):
    """(a) against (b): the scales of mpc_qp_soft_reference.ab_disagreement, but e relative to max(1, max e) of (b)."""
    rel = lambda x, y, sc: np.abs(x - y).max() / sc if y.size else 0.0
    ls = max(1.0, np.abs(r['Lam']).max()) if r['Lam'].size else 1.0
    es = max(1.0, np.abs(r['Eps']).max()) if r['Eps'].size else 1.0
    return dict(sol=max(rel(r['Xa'], r['X'], max(1.0, np.abs(r['X']).max())), rel(r['Ua'], r['U'], max(1.0, np.abs(r['U']).max()))),
                lam=rel(r['Lama'], r['Lam'], ls), e=rel(r['Epsa'], r['Eps'], es))


def closed_loop_quad(A, B, H, N, k0, x0, T, penalty, penalty2, W=None, **kw):
    """The receding-horizon loop on (b) -> dict X, U, nact, nviol [T] (stage 0), hres [T] = max(D z - d) of the applied step, usc [T] (its largest slack),
    margin, certificate.  W [T, nx]: a disturbance added to the plant step."""
    p = A.shape[0]
    D, d, rows = kw.get('D'), kw.get('d'), kw.get('rows')
    X = [np.asarray(x0, float)]; U = []; nact = []; nviol = []; hres = []; usc = []; margin = np.inf; cert = True
    for t in range(T):
        k = (k0 + t) % p
        r = solve_quad(A, B, H, N, k, X[-1], penalty, penalty2, **kw)
        u = r['U'][0]
        z = np.concatenate([X[-1], u])
        rk = int(D.shape[1] if rows is None else rows[k])
        hres.append((D[k, :rk] @ z - d[k, :rk]).max() if rk else -np.inf)
        usc.append(r['Eps'][0].max() if rk else 0.0)
        U.append(u); nact.append(r['nact0']); nviol.append(r['nviol0']); margin = min(margin, r['b']['margin'])
        cert = cert and r['b']['certificate'] and r['a']['status'] == 0
        X.append(A[k] @ X[-1] + B[k] @ u + (0.0 if W is None else W[t]))
    return dict(X=np.array(X), U=np.array(U), nact=np.array(nact), nviol=np.array(nviol), hres=np.array(hres), usc=np.array(usc), margin=margin, certificate=cert)


def kkt_check_quad(A, B, H, N, k0, X, U, Lam, Eps, penalty, penalty2, q=None, Pf=None, D=None, d=None, rows=None):
    """Solver-independent figures of a returned open-loop solution: dyn and stat of mpc_qp_reference.kkt_check (the adjoint recursion with the given lam),
    viol = max(D z - e - d) / max(1, |d|), low = min(lam, e), comp = max |lam (d - D z + e)| / max(1, max lam), and, relative to max(1, max lam),
    quad_v = max |lam - c - Z e| over the two-pair rows with e > 0 where lam exceeds c (violated), comp_e = max |e (c + Z e - lam)| over the two-pair rows,
    pure = max |e - lam / Z| max(1, Z) over the pure rows (|Z e - lam| where Z > 1)."""
    p = A.shape[0]
    base = mq.kkt_check(A, B, H, N, k0, X, U, Lam, q=q, Pf=Pf, D=D, d=d, rows=rows)
    viol, low, comp, comp_e, quad_v, pure_r = -np.inf, np.inf, 0.0, 0.0, 0.0, 0.0
    for j in range(N):
        k = (k0 + j) % p
        rk = int(D.shape[1] if rows is None else rows[k])
        if not rk:
            continue
        z = np.concatenate([X[j], U[j]])
        lam, e, c, Z = Lam[j, :rk], Eps[j, :rk], penalty[k, :rk], penalty2[k, :rk]
        _, two, pure, _ = kinds(c, Z)
        r = D[k, :rk] @ z - e - d[k, :rk]
        viol = max(viol, (r / np.maximum(1.0, np.abs(d[k, :rk]))).max())
        low = min(low, lam.min(), e.min())
        comp = max(comp, np.abs(lam * r).max())
        if two.any():
            nu = (c + Z * e - lam)[two]
            comp_e = max(comp_e, np.abs(e[two] * nu).max())
            vio = e[two] > np.abs(nu)
            if vio.any():
                quad_v = max(quad_v, np.abs(nu[vio]).max())
        if pure.any():
            pure_r = max(pure_r, (np.abs(e - lam / np.where(pure, Z, 1.0)) * np.maximum(1.0, Z))[pure].max())
    lmax = max(1.0, np.abs(Lam).max()) if Lam.size else 1.0
    return dict(dyn=base['dyn'], stat=base['stat'], viol=viol, low=low, comp=comp / lmax, comp_e=comp_e / lmax, quad_v=quad_v / lmax, pure=pure_r / lmax)


# ----------------------------------------------------------------------------- method (c): the slack as a pseudo-control
def lift_quad(A, B, H, penalty, penalty2, q=None, D=None, d=None, rows=None):
    """One problem -> dict A, B [p,nx,mb+nd], H [p,n+nd,n+nd], q [p,n+nd], D [p,2nd,n+nd], d [p,2nd], rows [p]: input mb + i of stage k is the slack of row i,
    with Z on its Hessian diagonal and c in q.  Rows of a stage: its D rows (with -e_i on the soft ones), then -e_i <= 0 of the two-pair ones.  Unused slack
    inputs get a unit Hessian, so they stay 0."""
    p, nx, mb = B.shape
    nd = D.shape[1]
    n = nx + mb
    rows = np.full(p, nd) if rows is None else np.asarray(rows)
    B2 = np.zeros((p, nx, mb + nd)); B2[:, :, :mb] = B
    H2 = np.zeros((p, n + nd, n + nd)); q2 = np.zeros((p, n + nd)); D2 = np.zeros((p, 2 * nd, n + nd)); d2 = np.zeros((p, 2 * nd)); r2 = np.zeros(p, int)
    for k in range(p):
        H2[k, :n, :n] = (H[k] + H[k].T) / 2
        if q is not None:
            q2[k, :n] = q[k]
        rk = int(rows[k])
        soft = [i for i in range(rk) if np.isfinite(penalty[k, i])]
        two = [i for i in soft if penalty[k, i] > 0]
        for i in range(nd):
            if i in soft:
                q2[k, n + i] = penalty[k, i]; H2[k, n + i, n + i] = penalty2[k, i]
            else:
                H2[k, n + i, n + i] = 1.0
        D2[k, :rk, :n] = D[k, :rk]; d2[k, :rk] = d[k, :rk]
        for i in soft:
            D2[k, i, n + i] = -1.0
        for o, i in enumerate(two):
            D2[k, rk + o, n + i] = -1.0
        r2[k] = rk + len(two)
    return dict(A=A, B=B2, H=H2, q=q2, D=D2, d=d2, rows=r2)


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}
CASES, SMALL = ms.CASES, ms.SMALL
L12 = [(f, zeta) for f in (0.3, 10.0) for zeta in (1.0, 100.0)]
PURE = (1e2, 1e3)
# (kind, case, f, zeta, first row of every stage hard): 'l12' c = f max lam, Z = zeta c; 'pure' c = 0, Z = f max lam
VARIANTS = ([('l12', c, f, z, False) for c in CASES for f, z in L12] + [('pure', c, f, 0.0, False) for c in CASES for f in PURE] +
            [('l12', mq.case_mixed_small, f, z, True) for f, z in L12] + [('pure', mq.case_mixed_small, f, 0.0, True) for f in PURE])
VARIANT_IDS = ['%s-%s-f%g%s%s' % (k, c.__name__, f, '-z%g' % z if k == 'l12' else '', '-mixed' if hf else '') for k, c, f, z, hf in VARIANTS]
INFEASIBLE = [(50.0, 500.0), (0.0, 500.0), (0.0, 5e5)]


def instances(kind, case, f, zeta=0.0, hard_first=False):
    """The instances of mpc_qp_soft_reference.instances (c = f max lam of the hard solution) with penalty, penalty2 of the variant."""
    key = ('inst', kind, case.__name__, f, zeta, hard_first)
    if key not in _CACHE:
        out = []
        for i in ms.instances(case, f, hard_first):
            i = dict(i)
            c = i['penalty']
            hard = ~np.isfinite(c)
            cf = np.where(hard, 0.0, c)
            if kind == 'l12':
                i['penalty2'] = zeta * cf
            else:
                i['penalty2'] = cf; i['penalty'] = np.where(hard, np.inf, 0.0)
            out.append(i)
        _CACHE[key] = out
    return _CACHE[key]


def solve_instances(kind, case, f, zeta=0.0, hard_first=False):
    key = ('solved', kind, case.__name__, f, zeta, hard_first)
    if key not in _CACHE:
        _CACHE[key] = [solve_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], i['penalty2'], **i['kw'])
                       for i in instances(kind, case, f, zeta, hard_first)]
    return _CACHE[key]


def infeasible_instance(c, Z):
    i = ms.infeasible_instance()
    i['penalty'] = np.full(i['penalty'].shape, c); i['penalty2'] = np.full(i['penalty'].shape, Z)
    return i


def batch_of(insts):
    """mpc_qp_soft_reference.batch_of with penalty2."""
    out = ms.batch_of(insts)
    out['penalty2'] = np.ascontiguousarray(np.stack([i['penalty2'] for i in insts]))
    return out
