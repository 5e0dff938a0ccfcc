"""Plain-numpy statement of the periodic optimal-control QP WITH SOFT AND QUADRATIC-SLACK ROWS (csrc/tmpc_periodic_qp.h, k_periodic_qp<true>): test
infrastructure of test_periodic_qp_soft_cpu.py / test_gpu_periodic_qp_soft*.py.  It imports periodic_qp_reference (pq) and changes nothing of it.

Per row of a stage, c = penalty and Z = penalty2 (the kinds of mpc_qp_quad_reference, read the same way):
    c = inf (Z = 0)   the hard row  D_i z <= d_i;
    c > 0, Z = 0      exact L1:  D_i z - e <= d_i, e >= 0, cost c e;
    c > 0, Z > 0      L1 + L2:   the same rows, cost c e + 1/2 Z e^2, stationarity in e: c + Z e - lam - nu = 0;
    c = 0, Z > 0      pure quadratic: D_i z - e <= d_i, cost 1/2 Z e^2, ONE complementarity pair (e = lam / Z >= 0 by itself).

(a) `ipm_soft`: the ELIMINATED iteration on pq.dense(...) -- the iteration of pq.ipm with the four row kinds; e and nu are eliminated per row and never
enter the linear system, which is the one of pq.newton_dense with another weight w and right-hand side beta on that row.  This is what the kernel runs.
    start      s = max(d, 1); hard and pure rows lam = 1; two-pair rows e = s, lam = nu = (c + Z e) / 2;
    residual   r_in = D z + s - d (hard),  D z - e + s - d (two pairs),  D z - lam / Z + s - d (pure); scaled by max(1, |d|);
    weights    hard:     w = lam / (s + RHO lam),               beta = r_in - s + c1 / lam,                        ds = -r_in - D dz + RHO dlam;
               L1:       w = 1 / (s / lam + e / nu + RHO),      beta = r_in - s + e + c1 / lam - c2 / nu,          de = -e + c2 / nu + (e / nu) dlam,  dnu = -dlam;
               L1 + L2:  nut = nu + Z e,  w = 1 / (s / lam + e / nut + RHO),  beta = r_in - s + c1 / lam + (e nu - c2) / nut,  de = (c2 - e nu + e dlam) / nut,
                         dnu = Z de - dlam;     both two-pair kinds: ds = -r_in - D dz + de + RHO dlam;
               pure:     rz = RHO + 1 / Z,  w = lam / (s + rz lam),  beta = r_in - s + c1 / lam,  ds = -r_in - D dz + rz dlam;
               every kind: dlam = w (D dz + beta);
    corrector  c1 = sigma mu - ds_aff dlam_aff,  c2 = sigma mu - de_aff dnu_aff (L1: = sigma mu + de_aff dlam_aff);
    mu, sigma  over every pair once: (sum s lam + sum_{two pairs} e nu) / (rows + two-pair rows); sigma = (mu_aff / mu)^3;
    step       one length min(1, 0.995 alpha_max) over s, lam and, on two-pair rows, e, nu;
    stop       that of pq.ipm; max lam is taken over lam alone.
    With every weight inf the statements executed are those of pq.ipm, in its order: the iterates are equal bit for bit (the CPU test holds that).
(b) `lift` + pq.polish: TRUTH.  Every soft row gets a pseudo-input e with a zero column in B, q_e = c, H_ee = Z; the rows are D z - e <= d, plus -e <= 0 on
    two-pair rows; a pseudo-input without a soft row is pinned by H_ee = 1 (its optimum is 0).  The lifted problem is solved by pq.polish at the active set
    that (a) found (row: lam > s; -e <= 0: nu > e) and checked with its certificate.  pq.ipm is NOT used on the lifted problem: the pseudo-inputs of L1
    rows have a zero Hessian and the Riccati pass of the hard iteration ends with status 2 there.
(c) `scalar_soft_closed_form`: nx = nu = p = N = 1 with the row u <= umax, extending pq.scalar_closed_form; f(u) is the cost with x = al u + be substituted:
    L1        u = umax if lam_hard <= c (lam_hard = -f'(umax)), else f'(u) + c = 0;
    L1 + L2   f'(u) + c + Z (u - umax) = 0 when that u exceeds umax (else the L1 answer u = umax);
    pure      f'(u) + Z (u - umax) = 0 when the free optimum exceeds umax.

Tolerances are measured, not chosen (test_periodic_qp_soft_cpu.py prints every figure and asserts the bound): PER_SOFT_IPM_VS_POLISH and PARITY below."""
import numpy as np

import mpc_qp_reference as mq
import periodic_qp_reference as pq

TOL, MAX_ITER, RHO = pq.TOL, pq.MAX_ITER, pq.RHO
MARGIN_MIN = pq.MARGIN_MIN
INF = np.inf
# (a) against (b) over CASES: X, U, eps relative to max(1, max|.|) of (b) (the slacks scaled like X); lam, nu, pi relative to max(1, max lam, max|nu|, max|pi|).
# Measured 4.97e-9, on lam of stage_shape (sol 6.9e-10, pi 6.4e-10, eps 1.4e-10 there; every other case stays below 1e-11: contradictory 9.8e-12 on X and eps,
# ragged_exact 2.2e-12 on lam); rounded up to one digit.  It is larger than pq.PER_IPM_VS_POLISH: at c of half the hard multipliers stage_shape has a weakly
# active hard-side row (stage 0, row 8: lam = 1.4e-2, next to the case's margin 1.1e-2) whose slack is still 6.9e-10 at the iterate that meets the stop rule
# (mu = 5.3e-14, r_p 1.1e-15, r_d 1.7e-15 after 9 iterations); one more iteration (tol 1e-12) brings the figure to 6.4e-11.
PER_SOFT_IPM_VS_POLISH = 5e-9
PARITY = 10 * PER_SOFT_IPM_VS_POLISH      # the GPU tests: the project's margin for another order of accumulation on the device


def kinds(P, pen, pen2):
    """c, Z per dense row (from [p, nd] arrays; None: c = 0 everywhere with pen2, Z = 0) -> c, Z, two (two pairs), pure, l2 (two pairs with Z > 0)."""
    p = len(pen if pen is not None else pen2)
    k = P['stage'] % p
    c = np.zeros(len(k)) if pen is None else np.asarray(pen, float)[k, P['row']]
    z = np.zeros(len(k)) if pen2 is None else np.asarray(pen2, float)[k, P['row']]
    two = (c < INF) & (c > 0)
    return c, z, two, c == 0.0, two & (z > 0)


def valid(pen, pen2):
    """The rule of the kernel over ALL entries of the [p, nd] arrays: Z >= 0 and finite, 0 on a hard row; c > 0, or c = 0 with Z > 0."""
    ref = pen if pen is not None else pen2
    c = np.zeros(np.shape(ref)) if pen is None else np.asarray(pen, float)
    z = np.zeros(np.shape(ref)) if pen2 is None else np.asarray(pen2, float)
    with np.errstate(invalid='ignore'):
        return bool(((z >= 0) & (z < INF)).all() and ((c > 0) | ((c == 0) & (z > 0))).all() and not ((c == INF) & (z != 0)).any())


def _newton(P, v, nue, piper, rdv, rpe, req, w, beta):
    """The linear system of pq.newton_dense with the row weights w and right-hand sides beta -> dv, G dv, dnue, dpi_per, or None."""
    Q, Cm, G, Je = P['Q'], P['Cm'], P['G'], P['Je']
    nv, nq = len(P['c']), len(P['b'])
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
    sol = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta) + Je.T @ (req / RHO)), -rpe]))
    dv = sol[:nv]
    return dv, G @ dv, (Je @ dv + req) / RHO, sol[nv:][-P['nx']:]


def ipm_soft(P, pen, pen2, tol=TOL, max_iter=MAX_ITER):
    """Method (a) -> dict v, lam, s, e, nu (of e >= 0), nue, pi, piper, iters, status, mu, rp, rd, eps (the reported slack: e, lam / Z on a pure row, 0 on a
    hard one), nviol, pcost, two, pure."""
    Q, c, Cm, b, G, h, Je, re = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h', 'Je', 're'))
    nv, m, nx, Nnx = len(c), len(h), P['nx'], P['N'] * P['nx']
    cc, zz, two, pure, l2 = kinds(P, pen, pen2)
    l1 = two & ~l2
    hard = ~two & ~pure
    n2 = int(two.sum())
    v = np.zeros(nv); s = np.maximum(P['d0'], 1.0) if m else np.zeros(0); lam = np.ones(m); nue = np.zeros(len(re)); piper = np.zeros(nx)
    e = np.where(two, s, 0.0)
    with np.errstate(all='ignore'):
        lam = np.where(two, 0.5 * (np.where(two, cc, 0.0) + zz * e), lam)
    nu = np.where(two, lam, 0.0)
    status, it = 1, 0
    mu = rp = rd = np.nan
    piv = np.zeros(Nnx)
    if not valid(pen, pen2):
        return dict(status=3, iters=0, v=v * np.nan, lam=lam * np.nan, eps=lam * np.nan, nviol=-1, two=two, pure=pure)
    rz = np.where(pure, RHO + 1.0 / np.where(pure, zz, 1.0), RHO)      # the dual regularisation of the row

    def direction(rpi, Gd, c1, c2):
        """w, beta of every row and, given G dv, the row directions dlam, ds, de, dnu."""
        with np.errstate(all='ignore'):
            nut = np.where(two, nu + zz * e, 1.0)
            w = np.where(two, 1.0 / (s / lam + e / nut + RHO), lam / (s + rz * lam))
            beta = rpi - s + c1 / lam
            beta = np.where(l1, rpi - s + e + c1 / lam - c2 / np.where(two, nu, 1.0), beta)
            beta = np.where(l2, rpi - s + c1 / lam + (e * nu - c2) / nut, beta)
            if Gd is None:
                return w, beta
            dl = w * (beta + Gd)
            de = np.where(l1, -e + c2 / np.where(two, nu, 1.0) + (e / np.where(two, nu, 1.0)) * dl, 0.0)
            de = np.where(l2, (c2 - e * nu + e * dl) / nut, de)
            ds = -rpi - Gd + de + rz * dl
            dnu = np.where(two, zz * de - dl, 0.0)
        return dl, ds, de, dnu

    def length(dl, ds, de, dnu):
        a = 1e300
        for x, dx, sel in ((s, ds, None), (lam, dl, None), (e, de, two), (nu, dnu, two)):
            neg = dx < 0 if sel is None else (dx < 0) & sel
            if neg.any():
                a = min(a, (-x[neg] / dx[neg]).min())
        return a

    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            g = Q @ v + c + G.T @ lam + Je.T @ nue
            piv = pq.adjoint(P, g, piper)
            rdv = g + Cm.T @ piv
            rpe = Cm @ v - b; req = Je @ v - re
            rpi = G @ v + s - h
            rpi = np.where(two, G @ v - e + s - h, rpi)
            rpi = np.where(pure, G @ v - lam / np.where(pure, zz, 1.0) + s - h, rpi)
            mu = (float(lam @ s) + float(e[two] @ nu[two]) if n2 else float(lam @ s)) / (m + n2) if m else 0.0
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
            zero = np.zeros(m)
            w, beta = direction(rpi, None, zero, zero)
            step = _newton(P, v, nue, piper, rdv, rpe, req, w, beta)
            if step is None:
                status = 2; break
            dv, Gd, dn, dp = step
            dl, ds, de, dnu = direction(rpi, Gd, zero, zero)
            if m:
                aa = min(1.0, length(dl, ds, de, dnu))
                comp = float((lam + aa * dl) @ (s + aa * ds))
                if n2:
                    comp += float((e[two] + aa * de[two]) @ (nu[two] + aa * dnu[two]))
                sigmu = (comp / (m + n2) / mu) ** 3 * mu
                c1 = sigmu - ds * dl; c2 = np.where(two, sigmu - de * dnu, 0.0)
                w, beta = direction(rpi, None, c1, c2)
                dv, Gd, dn, dp = _newton(P, v, nue, piper, rdv, rpe, req, w, beta)
                dl, ds, de, dnu = direction(rpi, Gd, c1, c2)
            al = min(1.0, mq.STEP_BACK * length(dl, ds, de, dnu))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; nue = nue + al * dn; piper = piper + al * dp
            e = e + al * de; nu = nu + al * dnu
    with np.errstate(all='ignore'):
        eps = np.where(two, e, np.where(pure, lam / np.where(pure, zz, 1.0), 0.0))
    soft = two | pure
    pcost = float(np.sum(np.where(soft, np.where(soft, cc, 0.0) * eps + 0.5 * zz * eps * eps, 0.0)))
    nviol = int((two & (e > nu)).sum() + (pure & (lam > s)).sum())
    return dict(v=v, lam=lam, s=s, e=e, nu=nu, nue=nue, pi=piv, piper=piper, iters=it, status=status, mu=mu, rp=rp, rd=rd, eps=eps, nviol=nviol, pcost=pcost,
                two=two, pure=pure, hard=hard)


def lift(A, B, H, periods, kw, pen, pen2):
    """The lifted problem of (b): nd pseudo-inputs per stage -> the arguments of pq.dense, and per phase the row numbers of the -e <= 0 rows."""
    A, B, H = (np.asarray(x, float) for x in (A, B, H))
    p, nx, nu = B.shape
    D, d = kw['D'], kw['d']
    nd = D.shape[1]
    n, nl = nx + nu, nx + nu + nd
    rows = np.full(p, nd) if kw.get('rows') is None else np.asarray(kw['rows'])
    cc = np.zeros((p, nd)) if pen is None else np.asarray(pen, float)
    zz = np.zeros((p, nd)) if pen2 is None else np.asarray(pen2, float)
    Bl = np.concatenate([B, np.zeros((p, nx, nd))], axis=2)
    Hl = np.zeros((p, nl, nl)); ql = np.zeros((p, nl))
    Dl = np.zeros((p, 2 * nd, nl)); dl = np.zeros((p, 2 * nd)); rl = np.zeros(p, int)
    pos = []
    for k in range(p):
        Hl[k, :n, :n] = 0.5 * (H[k] + H[k].T)
        if kw.get('q') is not None:
            ql[k, :n] = kw['q'][k]
        Dl[k, :rows[k], :n] = D[k, :rows[k]]; dl[k, :rows[k]] = d[k, :rows[k]]
        t = int(rows[k]); pk = {}
        for i in range(nd):
            soft = i < rows[k] and cc[k, i] < INF
            Hl[k, n + i, n + i] = zz[k, i] if soft else 1.0
            if soft:
                ql[k, n + i] = cc[k, i]
                Dl[k, i, n + i] = -1.0
                if cc[k, i] > 0:
                    Dl[k, t, n + i] = -1.0; pk[i] = t; t += 1
        rl[k] = t; pos.append(pk)
    Jl = None if kw.get('J') is None else np.concatenate([kw['J'], np.zeros(kw['J'].shape[:2] + (nd,))], axis=2)
    ndl = max(1, int(rl.max()))
    return dict(A=A, B=Bl, H=Hl, periods=periods, q=ql, c=kw.get('c'), D=Dl[:, :ndl], d=dl[:, :ndl], rows=rl, J=Jl, r=kw.get('r'), erows=kw.get('erows')), pos


def solve_soft(A, B, H, periods, kw, pen, pen2, tol=TOL, max_iter=MAX_ITER):
    """(a) then (b) -> dict a, P, Xa, Ua, Lama, Nua, Pia, Epsa of (a) and, when (a) converged, b (pq.polish of the lifted problem), X, U, Lam, Nu, Pi, Eps,
    cost (the total), pcost, active [N, nd] (the rows of D), nviol of (a)."""
    P = pq.dense(A, B, H, periods, **kw)
    a = ipm_soft(P, pen, pen2, tol, max_iter)
    out = dict(a=a, P=P)
    if 'nue' not in a:      # invalid weights: status 3 before the first iteration
        return out
    out['Xa'], out['Ua'], out['Lama'], out['Nua'], out['Pia'] = pq.unpack(P, a['v'], a['lam'], a['nue'], a['pi'])
    N, nd, nx, nu = P['N'], P['nd'], P['nx'], P['mb']
    Ea = np.zeros((N, nd)); Ea[P['stage'], P['row']] = a['eps']
    out['Epsa'] = Ea
    if a['status'] != 0:
        return out
    L, pos = lift(A, B, H, periods, kw, pen, pen2)
    PL = pq.dense(L['A'], L['B'], L['H'], L['periods'], q=L['q'], c=L['c'], D=L['D'], d=L['d'], rows=L['rows'], J=L['J'], r=L['r'], erows=L['erows'])
    p = len(L['rows'])
    rowact = np.zeros((N, nd), bool); rowact[P['stage'], P['row']] = a['lam'] > a['s']
    eact = np.zeros((N, nd), bool); eact[P['stage'], P['row']] = a['two'] & (a['nu'] > a['e'])
    act = np.zeros(len(PL['h']), bool)
    for t, (j, i) in enumerate(zip(PL['stage'], PL['row'])):
        k = j % p
        if i < nd and not any(i == r for r in pos[k].values()):
            act[t] = rowact[j, i]
        else:
            act[t] = eact[j, [s for s, r in pos[k].items() if r == i][0]]
    bb = pq.polish(PL, act)
    out['b'] = bb
    Xl, Ul, Laml, Nul, Pil = pq.unpack(PL, bb['v'], bb['lam'], bb['nue'], bb['pi'])
    out['X'], out['U'], out['Eps'], out['Nu'], out['Pi'] = Xl, Ul[:, :nu].copy(), Ul[:, nu:].copy(), Nul, Pil
    Lam = np.zeros((N, nd)); Lam[P['stage'], P['row']] = Laml[P['stage'], P['row']]
    out['Lam'] = Lam
    out['cost'] = float(0.5 * bb['v'] @ PL['Q'] @ bb['v'] + PL['c'] @ bb['v'])
    out['active'] = rowact
    return out


def ab_disagreement(r):
    """pq.ab_disagreement with the slacks scaled like X."""
    out = pq.ab_disagreement(r)
    out['eps'] = np.abs(r['Epsa'] - r['Eps']).max() / max(1.0, np.abs(r['Eps']).max()) if r['Eps'].size else 0.0
    return out


def tie_cpu_distance(c):
    """The fixed-point tie on the CPU: (a) of the periodic problem against (a) of the horizon-p MPC step from x*_0 with the terminal constraint x_N = x*_0 and
    the same penalty (mpc_qp_affine_reference.solve_aff) -> the worst distance of X, x_N, U, eps, scaled like ab_disagreement; None where that reference does
    not serve the rows (a Z > 0: it knows L1 rows only)."""
    import mpc_qp_affine_reference as af
    if c['pen2'] is not None and (c['pen2'] > 0).any():
        return None
    r, kw, p = solve_case(c), c['kw'], c['A'].shape[0]
    x0 = r['Xa'][0]
    m = af.solve_aff(c['A'], c['B'], c['H'], p, 0, x0, penalty=c['pen'], offset=kw.get('c'), trhs=np.tile(x0, (p, 1)), q=kw.get('q'), D=kw.get('D'), d=kw.get('d'),
                     rows=kw.get('rows'), J=kw.get('J'), r=kw.get('r'), erows=kw.get('erows'), Tx='constraint')
    assert m['a']['status'] == 0
    sx = max(1.0, np.abs(r['Xa']).max())
    return max(np.abs(m['Xa'][:p] - r['Xa']).max() / sx, np.abs(m['Xa'][p] - x0).max() / sx, np.abs(m['Ua'] - r['Ua']).max() / max(1.0, np.abs(r['Ua']).max()),
               np.abs(m['Epsa'] - r['Epsa']).max() / max(1.0, np.abs(r['Epsa']).max()))


def scalar_soft_closed_form(a, b, c, H, q, umax, pen, pen2=0.0):
    """nx = nu = p = N = 1 with u <= umax at the weights pen (c) and pen2 (Z) -> x, u, e, lam.  f(u) = 1/2 A2 u^2 + A1 u + const with x = al u + be."""
    al, be = b / (1.0 - a), c / (1.0 - a)
    A2 = al * al * H[0, 0] + 2.0 * al * H[0, 1] + H[1, 1]
    A1 = al * H[0, 0] * be + H[0, 1] * be + al * q[0] + q[1]
    uf = -A1 / A2
    if uf <= umax:
        return al * uf + be, uf, 0.0, 0.0
    lam_hard = -(A2 * umax + A1)
    if pen == INF:
        u = umax
    elif pen == 0.0:                       # pure: f'(u) + Z (u - umax) = 0
        u = (pen2 * umax - A1) / (A2 + pen2)
    elif lam_hard <= pen:
        u = umax
    else:                                  # f'(u) + c + Z (u - umax) = 0
        u = (pen2 * umax - A1 - pen) / (A2 + pen2)
    return al * u + be, u, u - umax, -(A2 * u + A1)


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def _hard_lam(case):
    """lam of the hard solution of a pq case, [p, nd] (the first period)."""
    c = case()
    r = pq.solve_case(c)
    return r['Lam'][:c['A'].shape[0]]


def _half(case):
    """c at half the hard multipliers; 1 on the rows whose hard multiplier is zero."""
    lam = _hard_lam(case)
    return np.where(lam > 0, 0.5 * lam, 1.0)


def _soft_case(name, base, pen, pen2, kw=None):
    if name not in _CACHE:
        c = base()
        _CACHE[name] = dict(name=name, A=c['A'], B=c['B'], H=c['H'], periods=c['periods'], kw=c['kw'] if kw is None else kw,
                            pen=None if pen is None else np.asarray(pen() if callable(pen) else pen, float),
                            pen2=None if pen2 is None else np.asarray(pen2() if callable(pen2) else pen2, float), base=c['name'])
    return _CACHE[name]


def case_scalar_l1():
    """scalar_bound, c at half the hard multiplier: the bound is violated."""
    return _soft_case('scalar_l1', pq.case_scalar_bound, lambda: _half(pq.case_scalar_bound), None)


def case_scalar_exact():
    """scalar_bound, c at 10 times the hard multiplier: the hard solution."""
    return _soft_case('scalar_exact', pq.case_scalar_bound, lambda: 10.0 * _hard_lam(pq.case_scalar_bound), None)


def case_scalar_l1l2():
    return _soft_case('scalar_l1l2', pq.case_scalar_bound, lambda: _half(pq.case_scalar_bound), [[2.0]])


def case_scalar_pure():
    return _soft_case('scalar_pure', pq.case_scalar_bound, None, [[5.0]])


def case_scalar_hard():
    return _soft_case('scalar_hard', pq.case_scalar_bound, [[INF]], None)


CONTRA_D = np.array([[-0.6, 0.3]])


def case_contradictory():
    """eig_one with d = [-0.6, 0.3]: x_1 <= -0.6 and x_1 >= -0.3; the L1 weight 50 on both rows."""
    kw = dict(pq.case_eig_one()['kw']); kw['d'] = CONTRA_D
    return _soft_case('contradictory', pq.case_eig_one, [[50.0, 50.0]], None, kw)


def _ragged_mixed():
    """The 4-row stage: hard, L1, L1 + L2, pure; the 1-row stage: L1."""
    h = _half(pq.case_ragged)
    pen = np.full((3, 4), INF); pen2 = np.zeros((3, 4))
    pen[1] = [INF, h[1, 1], h[1, 2], 0.0]; pen2[1] = [0.0, 0.0, 2.0, 5.0]
    pen[2, 0] = h[2, 0]
    return pen, pen2


def case_ragged():
    return _soft_case('ragged_mixed', pq.case_ragged, lambda: _ragged_mixed()[0], lambda: _ragged_mixed()[1])


def case_ragged_exact():
    """c = 10 max lam_hard on every row: the hard solution."""
    return _soft_case('ragged_exact', pq.case_ragged, lambda: np.full((3, 4), 10.0 * _hard_lam(pq.case_ragged).max()), None)


def case_wide_rows():
    return _soft_case('wide_rows', pq.case_wide_rows, lambda: _half(pq.case_wide_rows), None)


def case_odd():
    return _soft_case('odd', pq.case_odd, lambda: _half(pq.case_odd), lambda: np.full((4, 3), 2.0))


def case_two_periods():
    return _soft_case('two_periods', pq.case_two_periods, lambda: _ragged_mixed()[0], lambda: _ragged_mixed()[1])


def case_rolled():
    return _soft_case('rolled', pq.case_rolled, lambda: np.roll(_ragged_mixed()[0], 1, axis=0), lambda: np.roll(_ragged_mixed()[1], 1, axis=0))


def case_stage_shape():
    """nx 24 / nu 8 / p 6, 16 rows, c at half the hard multipliers: the only case with more than one 64-lane row chunk of the stage arrays."""
    return _soft_case('stage_shape', pq.case_stage_shape, lambda: _half(pq.case_stage_shape), None)


SCALAR_KINDS = [case_scalar_hard, case_scalar_l1, case_scalar_exact, case_scalar_l1l2, case_scalar_pure]
# Every case converges in (a) and carries a certificate with margin >= MARGIN_MIN in (b) (test_periodic_qp_soft_cpu.py asserts it): none was dropped.
CASES = SCALAR_KINDS + [case_contradictory, case_ragged, case_ragged_exact, case_wide_rows, case_odd, case_two_periods, case_rolled, case_stage_shape]
EXACT = [(case_scalar_exact, pq.case_scalar_bound), (case_ragged_exact, pq.case_ragged)]      # (the exact-penalty member, the hard case it reproduces)


def solve_case(c):
    key = ('solved', c['name'])
    if key not in _CACHE:
        _CACHE[key] = solve_soft(c['A'], c['B'], c['H'], c['periods'], c['kw'], c['pen'], c['pen2'])
    return _CACHE[key]


def batch_of(c):
    """A case -> the arguments of periodic_qp_batch with one member, penalty and penalty2 included."""
    out = pq.batch_of(dict(c, kw=c['kw']))
    one = lambda x: None if x is None else np.ascontiguousarray(x[None], float)
    out.update(penalty=one(c['pen']), penalty2=one(c['pen2']))
    return out


def many(nb=520, seed=43):
    """pq.many with the four kinds in turn, each with the bound active and inactive (member i: kind (i // 2) % 4 of hard, L1 at c = 0.6 |lam_hard| or 1, L1 + L2 with Z = 2, pure with Z = 5) -> batch
    arguments and the closed forms x, u, e [nb]."""
    if 'many' not in _CACHE:
        args, _, _, _ = pq.many(nb, seed)
        s = {k: args[k].reshape(nb, -1) for k in ('A', 'B', 'offset')}
        pen = np.zeros((nb, 1, 1)); pen2 = np.zeros((nb, 1, 1)); x = np.zeros(nb); u = np.zeros(nb); e = np.zeros(nb)
        for i in range(nb):
            a, b, c, H, q, umax = s['A'][i, 0], s['B'][i, 0], s['offset'][i, 0], args['H'][i, 0], args['q'][i, 0], args['d'][i, 0, 0]
            lam_hard = scalar_soft_closed_form(a, b, c, H, q, umax, INF)[3]
            kind = (i // 2) % 4
            pen[i] = INF if kind == 0 else (0.0 if kind == 3 else (0.6 * lam_hard if lam_hard > 0 else 1.0))
            pen2[i] = 2.0 if kind == 2 else (5.0 if kind == 3 else 0.0)
            x[i], u[i], e[i], _ = scalar_soft_closed_form(a, b, c, H, q, umax, pen[i, 0, 0], pen2[i, 0, 0])
        _CACHE['many'] = (dict(args, penalty=pen, penalty2=pen2), x, u, e)
    return _CACHE['many']
