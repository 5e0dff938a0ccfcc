"""Plain-numpy statement of the MPC step with SOFT inequality rows (exact L1 slack penalties; the reference's preprocessing.add_mpc_slacks seen through
pmpc.py).  Test infrastructure of test_mpc_qp_soft_cpu.py / test_gpu_mpc_qp_soft.py on top of mpc_qp_reference (imported, not changed):

    min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j + sum_{i soft} c_{k,i} e_{j,i}) + 1/2 x_N' Pf x_N,
    s.t. x_{j+1} = A_k x_j + B_k u_j,   D_{k,i} z_j - e_{j,i} <= d_{k,i}, e_{j,i} >= 0 (soft rows),   D_{k,i} z_j <= d_{k,i} (hard rows).

`penalty` [p, nd] describes the rows of one problem: +inf a hard row, a finite value > 0 a soft row with that weight.  On the dense problem of
mpc_qp_reference.dense it becomes one weight per row of G (`row_penalty`).

Method (a), `ipm_soft`: the interior-point iteration of mpc_qp_reference.ipm with the slack e and the multiplier nu of e >= 0 ELIMINATED per row, not lifted
into the variables.  A soft row carries two complementarity pairs, (s, lam) and (e, nu); stationarity in e reads c - lam - nu = 0.  The library runs the same
iteration stage by stage (csrc/tmpc_mpc_qp.h, the SOFT instantiation); the rules that define it are stated here and mirrored there:
    start      hard rows as before (s = max(d, 1), lam = 1); a soft row starts at s = max(d, 1), lam = nu = c / 2 and e = s, so that c - lam - nu = 0 holds and
               both pairs of the row carry the same complementarity product; dnu = -dlam and one step length keep c - lam - nu = 0 at every iterate (nu is
               kept as its own variable: c - lam would lose nu to cancellation when the row is violated);
    residual   r_in = D z - e + s - d of a soft row, scaled by max(1, |d|) like a hard row's;
    weights    eliminating ds, de, dnu from the row's Newton equations (D dz - de + ds - RHO dlam = -r_in, s dlam + lam ds = c1 - s lam,
               -e dlam + nu de = c2 - e nu) leaves dlam = w (D dz + beta),  w = 1 / (s / lam + e / nu + RHO),
               beta = r_in - s + e + c1 / lam - c2 / nu,  and then de = -e + c2 / nu + (e / nu) dlam,  ds = -r_in - D dz + de + RHO dlam.
               For a hard row (e = 0, no second pair) this is w = lam / (s + RHO lam): the same Newton system, another weight and right-hand side.  RHO plays
               the role it has there (w <= 1 / RHO when both s / lam and e / nu vanish, i.e. never for a soft row in practice: one of the two stays large);
    corrector  c1 = sigma mu - ds_aff dlam_aff,  c2 = sigma mu - de_aff dnu_aff = sigma mu + de_aff dlam_aff;
    mu, sigma  mu = (sum s lam + sum_{soft} e nu) / (rows + soft rows): every pair counts once; sigma = (mu_aff / mu)^3 with mu_aff counted the same way;
    step       alpha = min(1, 0.995 alpha_max) over s, lam and, on soft rows, e and nu;
    stop       as before; max lam is taken over lam alone (nu ~ c on every row that is not violated, and a threshold that grew with c would loosen the
               test on the hard-like pairs exactly in the exact-penalty regime).
Method (b), `polish_soft`: truth.  Every soft row is in one of three states -- inactive (lam = 0, e = 0, slack > 0), active (0 < lam < c, e = 0, D z = d),
violated (lam = c, e > 0, D z - e = d) --, hard rows keep their two; a row of stage 0 that acts on x_0 alone is a constant of the problem (violated by
-h where h < 0 and soft, inactive otherwise) and stays outside the solve; one dense KKT solve in (v, nu_dyn, lam_active, e_violated) and the certificate that every
strict inequality holds and stationarity is <= 1e-11.  `margin` is the smallest of the strict inequalities.
Method (c), `lift`: the slack as a pseudo-control (the reference's own form): e as extra inputs with zero columns in B and zero Hessian, cost c in q, rows
[D -I] <= d and -e <= 0, through the EXISTING hard iteration mpc_qp_reference.ipm (unused slack inputs get a unit Hessian, so they stay 0).

Penalties of the cases: f max lam of each instance's hard solution (1 where no row of the hard solution is active), f = 0.3 (some rows violated), 10 and 1e3
(the reference's factor: the exact-penalty regime, where the soft solution is the hard one).  Penalties are per problem, so every instance is its own problem
(`instances`)."""
import numpy as np

import lqr_horizon_reference as lh
import mpc_qp_reference as mq

# (a) against (b) over every case and factor below, relative to max(1, max|.|) of (b) (solution) and max(1, max lam) of (b) (lam, e).  Measured (the test
# test_mpc_qp_soft_cpu.py prints every figure): 2.6e-10 on the solution, 2.3e-9 on lam, 9.9e-12 on e; the smallest margin is 1.1e-3.  Rounded up to one digit.
SOFT_IPM_VS_POLISH = 3e-9
MARGIN_MIN = 1e-4
FACTORS = (0.3, 10.0, 1e3)
INACTIVE, ACTIVE, VIOLATED = 0, 1, 2


def row_penalty(P, penalty, k0):
    """penalty [p, nd] -> one weight per row of G of the dense problem P (inf: hard)."""
    if not len(P['h']):
        return np.zeros(0)
    p = penalty.shape[0]
    return np.array([penalty[(k0 + j) % p, i] for j, i in zip(P['stage'], P['row'])], float)


def ipm_soft(P, cvec, tol=mq.TOL, max_iter=mq.MAX_ITER):
    """Method (a) -> dict v, lam, s, e, nu, iters, status (0 converged, 1 max_iter, 2 not convex along the path, 3 non-finite), mu, rp, rd."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, m, ne = len(c), len(h), len(b)
    Nmb = P['N'] * P['mb']
    RHO = mq.RHO
    soft = np.isfinite(cvec)
    ms = int(soft.sum())
    Cx = Cm[:, Nmb:]
    Zn = np.concatenate([np.eye(Nmb), -np.linalg.solve(Cx, Cm[:, :Nmb])])
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0)
    lam = np.where(soft, 0.5 * np.where(soft, cvec, 0.0), 1.0); nu = np.where(soft, lam, 1.0)     # (nu of a hard row is a placeholder: never read)
    e = np.where(soft, s, 0.0)
    xs0 = np.abs(P['x0']).max()
    status, it = 1, 0
    mu = rp = rd = np.nan
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            g = Q @ v + c + G.T @ lam
            pi = np.linalg.solve(Cx.T, -g[Nmb:])
            rdv = g + Cm.T @ pi
            rpe = Cm @ v - b; rpi = G @ v - e + s - h
            mu = (float(lam @ s) + float(e[soft] @ nu[soft])) / (m + ms) if m else 0.0
            rp = max(np.abs(rpi / P['dscale']).max() if m else 0.0, np.abs(rpe).max() / max(1.0, xs0, np.abs(v[Nmb:]).max()))
            rd = np.abs(rdv[:Nmb]).max() / max(1.0, np.abs(g).max())
            lmax = lam.max() if m else 0.0
            if not np.isfinite([mu, rp, rd, lmax]).all():
                status = 3; break
            if rp <= tol and rd <= tol and mu <= mq.MU_FACTOR * tol * max(1.0, lmax):
                status = 0; break
            if it == max_iter:
                break
            w = np.where(soft, 1.0 / (s / lam + e / nu + RHO), lam / (s + RHO * lam))
            Kmat = np.block([[Q + G.T @ (w[:, None] * G), Cm.T], [Cm, np.zeros((ne, ne))]])
            if not np.isfinite(Kmat).all():
                status = 3; break
            red = Zn.T @ Kmat[:nv, :nv] @ Zn
            if np.linalg.eigvalsh(red).min() <= 0:
                status = 2; break

            def solve(c1, c2):
                beta = rpi - s + e + c1 / lam - np.where(soft, c2 / nu, 0.0)
                dv = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta)), -rpe]))[:nv]
                dl = w * (beta + G @ dv)
                de = np.where(soft, -e + c2 / nu + (e / nu) * dl, 0.0)
                return dv, dl, -rpi - G @ dv + de + RHO * dl, de

            def length(dl, ds, de):
                a = 1e300
                for x, dx in ((s, ds), (lam, dl), (e[soft], de[soft]), (nu[soft], -dl[soft])):
                    neg = dx < 0
                    if neg.any():
                        a = min(a, (-x[neg] / dx[neg]).min())
                return a
            z0 = np.zeros(m)
            dv, dl, ds, de = solve(z0, z0)
            if m:
                aa = min(1.0, length(dl, ds, de))
                mu_aff = (float((lam + aa * dl) @ (s + aa * ds)) + float((e + aa * de)[soft] @ (nu - aa * dl)[soft])) / (m + ms)
                sigmu = (mu_aff / mu) ** 3 * mu
                dv, dl, ds, de = solve(sigmu - ds * dl, sigmu + de * dl)
            al = min(1.0, mq.STEP_BACK * length(dl, ds, de))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; e = e + al * de; nu = nu - al * dl
    return dict(v=v, lam=lam, s=s, e=e, nu=np.where(soft, nu, 0.0), iters=it, status=status, mu=mu, rp=rp, rd=rd)


def states_of(a, cvec):
    """The three-state pattern of an iterate of (a): violated where a soft row has e > nu, else active where lam > s, else inactive."""
    soft = np.isfinite(cvec)
    st = np.where(a['lam'] > a['s'], ACTIVE, INACTIVE)
    st[soft & (a['e'] > a['nu'])] = VIOLATED
    return st


def polish_soft(P, cvec, state):
    """Method (b): the rows with state ACTIVE as equalities, those with state VIOLATED as equalities with their slack free and lam = c -> dict v, lam, e (all
    rows), slack = h - G v + e, certificate, margin, stat."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, ne = len(c), len(b)
    state = np.array(state)
    fixed = ~G.any(axis=1)                                                   # rows on x_0 alone: constants of the problem, outside the KKT system
    state[fixed] = np.where(np.isfinite(cvec[fixed]) & (h[fixed] < 0), VIOLATED, INACTIVE)
    act, vio = (state == ACTIVE) & ~fixed, (state == VIOLATED) & ~fixed
    if ((state == VIOLATED) & ~np.isfinite(cvec)).any():
        raise ValueError('polish_soft: a hard row cannot be violated')
    Ga, Gv = G[act], G[vio]
    na, nvio = Ga.shape[0], Gv.shape[0]
    nt = nv + ne + na + nvio
    K = np.zeros((nt, nt))
    K[:nv, :nv] = Q; K[:nv, nv:nv + ne] = Cm.T; K[nv:nv + ne, :nv] = Cm
    K[:nv, nv + ne:nv + ne + na] = Ga.T; K[nv + ne:nv + ne + na, :nv] = Ga
    r = slice(nv + ne + na, nt)
    K[r, :nv] = Gv; K[r, r] = -np.eye(nvio)
    sol = np.linalg.solve(K, np.concatenate([-c - Gv.T @ cvec[vio], b, h[act], h[vio]]))
    v, pi = sol[:nv], sol[nv:nv + ne]
    lam = np.zeros(len(h)); lam[act] = sol[nv + ne:nv + ne + na]; lam[vio] = cvec[vio]
    e = np.zeros(len(h)); e[vio] = sol[r]
    fv = fixed & (state == VIOLATED)
    lam[fv] = cvec[fv]; e[fv] = -h[fv]; vio = vio | fv
    slack = h - G @ v + e
    grad = Q @ v + c
    stat = np.abs(grad + Cm.T @ pi + G.T @ lam).max() / max(1.0, np.abs(grad).max())
    strict = [slack[state == INACTIVE], lam[act], (cvec - lam)[act], e[vio]]            # (c - lam = inf on a hard row)
    margin = min([x.min() for x in strict if x.size] + [np.inf])
    return dict(v=v, lam=lam, e=e, slack=slack, stat=stat, margin=margin, certificate=bool(margin > 0 and stat <= 1e-11), nact=int(na + vio.sum()), nviol=int(vio.sum()), state=state)


def solve_soft(A, B, H, N, k0, x0, penalty, tol=mq.TOL, max_iter=mq.MAX_ITER, **kw):
    """(a) then (b) on one instance (penalty [p, nd]) -> dict a, b, state, X, U, Lam, Eps of (b), Xa, Ua, Lama, Epsa of (a), nact0 / nviol0 (rows of stage 0
    that are not inactive / that are violated), P, cvec."""
    P = mq.dense(A, B, H, N, k0, x0, **kw)
    cvec = row_penalty(P, penalty, k0)
    a = ipm_soft(P, cvec, tol, max_iter)
    st = states_of(a, cvec)
    bb = polish_soft(P, cvec, st)
    st = bb['state']
    X, U, Lam = mq.unpack(P, bb['v'], bb['lam'])
    Xa, Ua, Lama = mq.unpack(P, a['v'], a['lam'])
    s0 = P['stage'] == 0
    return dict(a=a, b=bb, state=st, X=X, U=U, Lam=Lam, Eps=mq.unpack(P, bb['v'], bb['e'])[2], Xa=Xa, Ua=Ua, Lama=Lama, Epsa=mq.unpack(P, a['v'], a['e'])[2],
                State=mq.unpack(P, bb['v'], st.astype(float))[2].astype(int), nact0=int((s0 & (st != INACTIVE)).sum()), nviol0=int((s0 & (st == VIOLATED)).sum()),
                P=P, cvec=cvec)


def ab_disagreement(r):
    """(a) against (b): the solution relative to max(1, max|.|) of (b), lam and e relative to max(1, max lam) of (b)."""
    rel = lambda x, y, sc: np.abs(x - y).max() / sc if y.size else 0.0
    ls = max(1.0, np.abs(r['Lam']).max()) if r['Lam'].size else 1.0
    return dict(sol=max(rel(r['Xa'], r['X'], max(1.0, np.abs(r['X']).max())), rel(r['Ua'], r['U'], max(1.0, np.abs(r['U']).max()))),
                lam=rel(r['Lama'], r['Lam'], ls), e=rel(r['Epsa'], r['Eps'], ls))


def closed_loop_soft(A, B, H, N, k0, x0, T, penalty, **kw):
    """The receding-horizon loop on (b) -> dict X, U, nact, nviol [T] (stage 0), hres [T] = max(D z - d) of the applied step, usc [T] (its largest slack),
    margin, certificate."""
    p = A.shape[0]
    D, d, rows = kw.get('D'), kw.get('d'), kw.get('rows')
    X = [np.asarray(x0, float)]; U = []; nact = []; nviol = []; hres = []; usc = []; margin = np.inf; cert = True
    for t in range(T):
        k = (k0 + t) % p
        r = solve_soft(A, B, H, N, k, X[-1], penalty, **kw)
        u = r['U'][0]
        z = np.concatenate([X[-1], u])
        rk = int(D.shape[1] if rows is None else rows[k])
        hres.append((D[k, :rk] @ z - d[k, :rk]).max() if rk else -np.inf)
        usc.append(r['Eps'][0].max() if rk else 0.0)
        U.append(u); nact.append(r['nact0']); nviol.append(r['nviol0']); margin = min(margin, r['b']['margin'])
        cert = cert and r['b']['certificate'] and r['a']['status'] == 0
        X.append(A[k] @ X[-1] + B[k] @ u)
    return dict(X=np.array(X), U=np.array(U), nact=np.array(nact), nviol=np.array(nviol), hres=np.array(hres), usc=np.array(usc), margin=margin, certificate=cert)


def kkt_check_soft(A, B, H, N, k0, X, U, Lam, Eps, penalty, q=None, Pf=None, D=None, d=None, rows=None):
    """Solver-independent figures of a returned open-loop solution with slacks: dyn and stat of mpc_qp_reference.kkt_check (the adjoint recursion with the given
    lam), viol = max(D z - e - d) / max(1, |d|), low = min(lam, c - lam, e) (>= 0 up to rounding), comp = max |lam (d - D z + e)| / max(1, max lam) and
    comp_e = max |e (c - lam)| / max(1, max lam) over the soft rows."""
    p, nx = A.shape[0], A.shape[1]
    base = mq.kkt_check(A, B, H, N, k0, X, U, Lam, q=q, Pf=Pf, D=D, d=d, rows=rows)
    viol, low, comp, comp_e = -np.inf, np.inf, 0.0, 0.0
    for j in range(N):
        k = (k0 + j) % p
        rk = int(D.shape[1] if rows is None else rows[k])
        if not rk:
            continue
        z = np.concatenate([X[j], U[j]])
        lam, e, c = Lam[j, :rk], Eps[j, :rk], penalty[k, :rk]
        r = D[k, :rk] @ z - e - d[k, :rk]
        viol = max(viol, (r / np.maximum(1.0, np.abs(d[k, :rk]))).max())
        soft = np.isfinite(c)
        low = min(low, lam.min(), e.min(), (c - lam)[soft].min() if soft.any() else np.inf)
        comp = max(comp, np.abs(lam * r).max())
        comp_e = max(comp_e, np.abs(e[soft] * (c - lam)[soft]).max() if soft.any() else 0.0)
    lmax = max(1.0, np.abs(Lam).max()) if Lam.size else 1.0
    return dict(dyn=base['dyn'], stat=base['stat'], viol=viol, low=low, comp=comp / lmax, comp_e=comp_e / lmax)


# ----------------------------------------------------------------------------- method (c): the slack as a pseudo-control
def lift(A, B, H, penalty, q=None, D=None, d=None, rows=None):
    """One problem (A [p,nx,nx], B [p,nx,mb], H [p,n,n], penalty [p,nd], ...) -> dict A, B [p,nx,mb+nd], H [p,n+nd,n+nd], q [p,n+nd], D [p,2nd,n+nd], d [p,2nd],
    rows [p]: input mb + i of stage k is the slack of row i.  Rows of a stage: its D rows (with -e_i on the soft ones), then -e_i <= 0 of the soft ones."""
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
        for i in range(nd):
            if i in soft:
                q2[k, n + i] = penalty[k, i]
            else:
                H2[k, n + i, n + i] = 1.0
        D2[k, :rk, :n] = D[k, :rk]; d2[k, :rk] = d[k, :rk]
        for i in soft:
            D2[k, i, n + i] = -1.0
        for o, i in enumerate(soft):
            D2[k, rk + o, n + i] = -1.0
        r2[k] = rk + len(soft)
    return dict(A=A, B=B2, H=H2, q=q2, D=D2, d=d2, rows=r2)


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def case_infeasible_when_hard():
    """p 3 / nx 3 / nu 1, N = 5 from phase 2, rows +-x_1 <= 0.1 on the first state, x_0 = (1, 0.2, -0.3): no feasible point when the rows are hard."""
    if 'infeasible' not in _CACHE:
        base = lh.case_no_rows()
        A, B, H = base['A'][:1], base['B'][:1], base['Hc'][:1]
        nb, p, nx, _ = A.shape
        n = nx + B.shape[3]
        D = np.zeros((1, p, 2, n)); D[:, :, 0, 0] = 1.0; D[:, :, 1, 0] = -1.0
        _CACHE['infeasible'] = dict(A=A, B=B, H=H, Pf=np.ascontiguousarray(np.broadcast_to(np.eye(nx), (1, p, nx, nx))), X0=np.array([[[1.0, 0.2, -0.3]]]), N=5, k0=2,
                                    q=None, ncnt=None, D=D, d=np.full((1, p, 2), 0.1), rows=np.full((1, p), 2), penalty=np.full((1, p, 2), 50.0))
    return _CACHE['infeasible']


def case_mixed_small_N2():
    return mq.case_mixed_small(2)


CASES = [mq.case_box_nu1, mq.case_box_nu2, mq.case_mixed_small, case_mixed_small_N2, mq.case_single_phase, mq.case_box_bench, mq.case_mixed_bench]
SMALL = [mq.case_box_nu1, mq.case_box_nu2, mq.case_mixed_small]
# (case, factor, first row of every stage hard)
VARIANTS = [(c, f, False) for c in CASES for f in FACTORS] + [(mq.case_mixed_small, f, True) for f in FACTORS]
VARIANT_IDS = ['%s-f%g%s' % (c.__name__, f, '-mixed' if hf else '') for c, f, hf in VARIANTS]


def instances(case, f, hard_first=False):
    """Every (member, state) of a case as its own problem with its own penalty f max lam (of its hard solution; 1 where nothing is active) ->
    list of dicts A, B, H [p,..], N, k0, x0, kw (q, Pf, D, d, rows), penalty [p, nd], hard (the dict of mpc_qp_reference.solve)."""
    key = ('inst', case.__name__, f, hard_first)
    if key not in _CACHE:
        c = case()
        hard = mq.solve_case(c)
        out = []
        for b in range(c['A'].shape[0]):
            for s, x0 in enumerate(c['X0'][b]):
                lmax = hard[b][s]['Lam'].max() if hard[b][s]['Lam'].size else 0.0
                pen = np.full(c['d'][b].shape, f * (lmax if lmax > 0 else 1.0))
                if hard_first:
                    pen[:, 0] = np.inf
                out.append(dict(A=c['A'][b], B=c['B'][b], H=c['H'][b], N=c['N'], k0=c['k0'], x0=x0, kw=mq.kwargs(c, b), penalty=pen, hard=hard[b][s]))
        _CACHE[key] = out
    return _CACHE[key]


def solve_instances(case, f, hard_first=False):
    """`instances` through (a) and (b), once per process -> list of the dicts of solve_soft."""
    key = ('solved', case.__name__, f, hard_first)
    if key not in _CACHE:
        _CACHE[key] = [solve_soft(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], i['penalty'], **i['kw']) for i in instances(case, f, hard_first)]
    return _CACHE[key]


def infeasible_instance():
    c = case_infeasible_when_hard()
    return dict(A=c['A'][0], B=c['B'][0], H=c['H'][0], N=c['N'], k0=c['k0'], x0=c['X0'][0, 0], kw=mq.kwargs(c, 0), penalty=c['penalty'][0])


def batch_of(insts):
    """A list of instances of one shape -> batched arrays (one problem per instance, ns = 1): dict A, B, H, X0, q, Pf, D, d, ndcnt, penalty, N, k0."""
    st = lambda k: np.ascontiguousarray(np.stack([i[k] for i in insts]))
    kw = lambda k: None if insts[0]['kw'][k] is None else np.ascontiguousarray(np.stack([np.asarray(i['kw'][k]) for i in insts]))
    return dict(A=st('A'), B=st('B'), H=st('H'), X0=st('x0')[:, None], q=kw('q'), Pf=kw('Pf'), D=kw('D'), d=kw('d'), ndcnt=kw('rows').astype(np.int32),
                penalty=st('penalty'), N=insts[0]['N'], k0=insts[0]['k0'])
