"""Plain-numpy statement of the WARM START of the constrained MPC step (test infrastructure of test_mpc_qp_warm_cpu.py / test_gpu_mpc_qp_warm*.py on top of
mpc_qp_reference, mpc_qp_soft_reference, mpc_qp_eq_reference, mpc_qp_affine_reference and mpc_qp_quad_reference, which are imported, not changed).

`ipm_warm` is the iteration of the four references restated once with the start injected: on hard rows it is mpc_qp_reference.ipm, with a penalty
ipm_soft, with equality / terminal rows (and the affine vectors in b, c, re) ipm_eq, with penalty2 ipm_quad; without a start it is their cold start.
A start is the stage-wise tuple the library returns: X [N+1,nx], U [N,mb], Lam [N,nd], Eps [N,nd], Nu [N,ne], NuT [nt].  s and the multiplier nu of e >= 0 are
NOT part of it: the floors derive them.  "Previous" is the converged iterate of the preceding solve, delta is `warm_floor` (csrc/tmpc_mpc_qp.h, the WARM
instantiations, mirrors the rule):

  shift by one stage (shift = 1: the loop, or a guess from the previous phase)
      new stage j takes old stage j + 1 for j <= N - 2 (its phase and therefore its rows are the same); x_0 is the measured state;
      x_1 .. x_{N-1} are the old predictions x_2 .. x_N; u_{N-1} repeats the old last input; x_N = A_k x_{N-1} + B_k u_{N-1} (+ c_k) at the phase k of the
      new last stage; lam, e, the equality multipliers shift the same way, the new last stage gets zeros before the floors; nu_T is kept;
  no shift (shift = 0: a guess for the same phase)   everything as given, x_0 replaced;
  floors by row kind, all directions zero
      hard row        s = max(d - D z, delta),  lam = max(lam, delta);
      L1 and L1 + L2  e = max(e, delta);  lam = clip(lam, delta, c + Z e - delta),  nu = c + Z e - lam  (c + Z e - lam - nu = 0 holds exactly);
                      a row with c + Z e < 2 delta takes its cold value lam = nu = (c + Z e) / 2;  s = max(d - D z + e, delta);
      pure quadratic  lam = max(lam, delta),  s = max(d - D z + lam / Z, delta)  (the guess's eps = lam / Z is not read);
      equality and terminal multipliers: free, no floor;
  fallbacks
      a guess with a non-finite entry (a failed predecessor returns NaN) starts cold: warm code 0;
      a warm-started solve that ends with status 1 or 2 is solved again from the cold start and `iters` counts both attempts: warm code 2 (an infeasible
      instance therefore costs two runs of max_iter); status 3 is not retried; a step that fails for good has warm code -1;
  default floor delta = 1e-2, absolute.

`closed_loop_warm` is the receding-horizon loop on the ITERATES (the library applies u_0 of its iterate, and the next start is the shifted iterate), with
the plant, disturbance and callback of the library's loops."""
import numpy as np

import mpc_qp_reference as mq
import mpc_qp_soft_reference as ms
import mpc_qp_eq_reference as eqr
import mpc_qp_affine_reference as afr
import mpc_qp_quad_reference as mqq

WARM_FLOOR = 1e-2
COLD, WARM, RETRIED, FAILED = 0, 1, 2, -1


def weights(P, k0, penalty=None, penalty2=None):
    """penalty, penalty2 [p, nd] or None -> (cvec, zvec) per row of G (inf / 0: a hard row)."""
    m = len(P['h'])
    cvec = ms.row_penalty(P, penalty, k0) if penalty is not None and m else np.full(m, np.inf)
    zvec = ms.row_penalty(P, penalty2, k0) if penalty2 is not None and m else np.zeros(m)
    return cvec, zvec


def cold_start(P, cvec, zvec):
    """The start of the four references -> dict v, lam, s, e, nu, nue."""
    m = len(P['h'])
    _, two, _, quad = mqq.kinds(cvec, zvec)
    zz = np.where(quad, zvec, 0.0)
    s = np.maximum(P['d0'], 1.0) if m else np.zeros(0)
    e = np.where(two, s, 0.0)
    lam = np.where(two, 0.5 * (np.where(two, cvec, 0.0) + zz * e), 1.0)
    return dict(v=np.zeros(len(P['c'])), lam=lam, s=s, e=e, nu=np.where(two, lam, 1.0), nue=np.zeros(len(P.get('re', ()))))


def shift_guess(guess, x0, A, B, k0, offset=None, shift=1):
    """The stage-wise shift (k0: the phase of the NEW problem) -> dict X, U, Lam, Eps, Nu, NuT; arrays that the guess lacks stay None."""
    X, U = np.array(guess['X'], float), np.array(guess['U'], float)
    N, p = U.shape[0], A.shape[0]
    opt = {k: None if guess.get(k) is None else np.array(guess[k], float) for k in ('Lam', 'Eps', 'Nu', 'NuT')}
    if shift:
        X = np.concatenate([X[1:], X[-1:]]); U = np.concatenate([U[1:], U[-1:]])
        for k in ('Lam', 'Eps', 'Nu'):
            if opt[k] is not None:
                opt[k] = np.concatenate([opt[k][1:], np.zeros_like(opt[k][:1])])
    X[0] = x0
    if shift:
        k = (k0 + N - 1) % p
        X[N] = A[k] @ X[N - 1] + B[k] @ U[N - 1] + (0.0 if offset is None else offset[k])
    return dict(X=X, U=U, **opt)


def warm_start(P, cvec, zvec, g, floor=WARM_FLOOR, relative=False):
    """The floors on a (shifted) stage-wise guess g of the dense problem P -> the start dict of cold_start."""
    m, N, mb = len(P['h']), P['N'], P['mb']
    if relative:                                                            # (not the library's rule: the alternative the default was weighed against,
        floor = floor * P['dscale'] if m else floor                         #  delta max(1, |d_i|) per row; scripts/mpc_qp_warm_reference_counts.py)
    hard, two, pure, quad = mqq.kinds(cvec, zvec)
    v = np.concatenate([g['U'].reshape(-1), g['X'][1:].reshape(-1)])
    pick = lambda a: a[P['stage'], P['row']] if a is not None and m else np.zeros(m)
    lam, e = pick(g['Lam']), np.where(two, pick(g['Eps']), 0.0)
    dz = P['h'] - P['G'] @ v if m else np.zeros(0)                            # d - D z of every row
    e = np.where(two, np.maximum(e, floor), 0.0)
    tot = np.where(two, np.where(two, cvec, 0.0) + np.where(quad, zvec, 0.0) * e, 0.0)
    lam2 = np.where(tot < 2 * floor, 0.5 * tot, np.minimum(np.maximum(lam, floor), tot - floor))
    lam = np.where(two, lam2, np.maximum(lam, floor))
    nu = np.where(two, tot - lam, 1.0)
    zinv = np.where(pure, 1.0 / np.where(pure, zvec, 1.0), 0.0)
    s = np.maximum(dz + e + lam * zinv, floor)
    nue = np.zeros(len(P.get('re', ())))
    if len(nue):
        ms_ = len(P['estage'])
        if ms_:
            nue[:ms_] = g['Nu'][P['estage'], P['erow']]
        if P['nt']:
            nue[ms_:] = g['NuT']
    return dict(v=v, lam=lam, s=s, e=e, nu=nu, nue=nue)


def ipm_warm(P, cvec, zvec, start=None, tol=mq.TOL, max_iter=mq.MAX_ITER):
    """The iteration of ipm / ipm_soft / ipm_eq / ipm_quad from `start` (None: cold) -> dict v, lam, s, e (lam / Z on pure rows), nu, nue, iters, status, mu,
    rp, rd."""
    Q, c, Cm, b, G, h = (P[k] for k in ('Q', 'c', 'Cm', 'b', 'G', 'h'))
    nv, m, ne = len(c), len(h), len(b)
    Je, re = P.get('Je', np.zeros((0, nv))), P.get('re', np.zeros(0))
    term = P['escale'] == 0.0 if 'escale' in P else np.zeros(0, bool)
    Js = np.where(term[:, None], 0.0, Je)
    Nmb = P['N'] * P['mb']
    RHO = mq.RHO
    hard, two, pure, quad = mqq.kinds(cvec, zvec)
    mp = m + int(two.sum())
    zz = np.where(quad, zvec, 0.0)
    zinv = np.where(pure, 1.0 / np.where(pure, zvec, 1.0), 0.0)
    rz = RHO + zinv
    Cx = Cm[:, Nmb:]
    Zn = np.concatenate([np.eye(Nmb), -np.linalg.solve(Cx, Cm[:, :Nmb])])
    st = cold_start(P, cvec, zvec) if start is None else start
    v, lam, s, e, nu, nue = (np.array(st[k], float) for k in ('v', 'lam', 's', 'e', 'nu', 'nue'))
    xs0 = np.abs(P['x0']).max()
    status, it = 1, 0
    mu = rp = rd = np.nan
    with np.errstate(all='ignore'):
        for it in range(max_iter + 1):
            gs = Q @ v + c + G.T @ lam + Js.T @ nue
            g = gs + (Je - Js).T @ nue
            pi = np.linalg.solve(Cx.T, -g[Nmb:])
            rdv = g + Cm.T @ pi
            rpe = Cm @ v - b; rpi = G @ v - np.where(pure, lam * zinv, e) + s - h; req = Je @ v - re
            mu = (float(lam @ s) + float(e[two] @ nu[two])) / mp if m else 0.0
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
            nt = nu + zz * e
            enu = np.where(quad, e * nu / nt, e)
            w = np.where(two, 1.0 / (s / lam + e / nt + RHO), lam / (s + rz * lam))
            Kmat = np.block([[Q + G.T @ (w[:, None] * G) + Je.T @ Je / RHO, Cm.T], [Cm, np.zeros((ne, ne))]])
            if not np.isfinite(Kmat).all():
                status = 3; break
            red = Zn.T @ Kmat[:nv, :nv] @ Zn
            if np.linalg.eigvalsh(red).min() <= 0:
                status = 2; break

            def solve(c1, c2):
                beta = rpi - s + enu + c1 / lam - np.where(two, c2 / nt, 0.0)
                dv = np.linalg.solve(Kmat, np.concatenate([-(rdv + G.T @ (w * beta) + Je.T @ (req / RHO)), -rpe]))[:nv]
                dl = w * (beta + G @ dv)
                de = np.where(two, -enu + c2 / nt + (e / nt) * dl, 0.0)
                return dv, dl, -rpi - G @ dv + de + rz * dl, de, zz * de - dl, (Je @ dv + req) / RHO

            def length(dl, ds, de, dn):
                a = 1e300
                for x, dx in ((s, ds), (lam, dl), (e[two], de[two]), (nu[two], dn[two])):
                    neg = dx < 0
                    if neg.any():
                        a = min(a, (-x[neg] / dx[neg]).min())
                return a
            z0 = np.zeros(m)
            dv, dl, ds, de, dn, dq = solve(z0, z0)
            if m:
                aa = min(1.0, length(dl, ds, de, dn))
                mu_aff = (float((lam + aa * dl) @ (s + aa * ds)) + float((e + aa * de)[two] @ (nu + aa * dn)[two])) / mp
                sigmu = (mu_aff / mu) ** 3 * mu
                dv, dl, ds, de, dn, dq = solve(sigmu - ds * dl, sigmu - de * dn)
            al = min(1.0, mq.STEP_BACK * length(dl, ds, de, dn))
            v = v + al * dv; lam = lam + al * dl; s = s + al * ds; e = e + al * de; nu = nu + al * dn; nue = nue + al * dq
    return dict(v=v, lam=lam, s=s, e=np.where(pure, lam * zinv, e), nu=np.where(two, nu, 0.0), nue=nue, iters=it, status=status, mu=mu, rp=rp, rd=rd)


def dense_of(A, B, H, N, k0, x0, kw):
    """The dense problem of one step; kw: q, Pf, D, d, rows, J, r, erows, Tx, offset, qf, trhs (each optional)."""
    return afr.dense_aff(A, B, H, N, k0, x0, kw.get('offset'), kw.get('qf'), kw.get('trhs'), **{k: kw.get(k) for k in ('q', 'Pf', 'D', 'd', 'rows', 'J', 'r', 'erows', 'Tx')})


def stagewise(P, a):
    """An iterate of ipm_warm -> the stage-wise dict X, U, Lam, Eps, Nu, NuT (the library's X, U, lam, eps, nu, nu_term)."""
    X, U, Lam = mq.unpack(P, a['v'], a['lam'])
    Nu, NuT = eqr.unpack_nu(P, a['nue']) if 'estage' in P else (np.zeros((P['N'], 0)), np.zeros(0))
    return dict(X=X, U=U, Lam=Lam, Eps=mq.unpack(P, a['v'], a['e'])[2], Nu=Nu, NuT=NuT)


def solve_warm(A, B, H, N, k0, x0, guess=None, shift=0, floor=WARM_FLOOR, penalty=None, penalty2=None, tol=mq.TOL, max_iter=mq.MAX_ITER, relative=False, **kw):
    """One step from a stage-wise guess (None: cold) with the fallbacks -> dict a (the iterate that delivered), start (the warm start that was tried, or None),
    warm (the code), iters (both attempts), status, P, cvec, zvec and the stage-wise X, U, Lam, Eps, Nu, NuT (NaN when the step failed)."""
    P = dense_of(A, B, H, N, k0, x0, kw)
    cvec, zvec = weights(P, k0, penalty, penalty2)
    start = None
    if guess is not None and all(np.isfinite(np.asarray(v, float)).all() for v in guess.values() if v is not None):      # (the guess as given: before the shift)
        start = warm_start(P, cvec, zvec, shift_guess(guess, x0, A, B, k0, kw.get('offset'), shift), floor, relative)
    a = ipm_warm(P, cvec, zvec, start, tol, max_iter)
    code, iters = (WARM if start is not None else COLD), a['iters']
    if start is not None and a['status'] in (1, 2):
        a = ipm_warm(P, cvec, zvec, None, tol, max_iter)
        code, iters = RETRIED, iters + a['iters']
    out = dict(a=a, start=start, warm=code if a['status'] == 0 else FAILED, iters=iters, status=a['status'], P=P, cvec=cvec, zvec=zvec)
    sw = stagewise(P, a)
    out.update({k: v if a['status'] == 0 else np.full(v.shape, np.nan) for k, v in sw.items()})
    return out


def closed_loop_warm(A, B, H, N, k0, x0, T, warm=True, guess=None, guess_shift=0, floor=WARM_FLOOR, plant=None, W=None, callback=None, **kw):
    """The receding-horizon loop on the iterates: step t solves from phase (k0 + t) mod p, from the shifted iterate of step t - 1 (warm) or cold, applies u_0 to
    x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t (plant None: the model) or to callback(t, x, u_0) -> dict X [T+1,nx], U [T,mb], iters, warm [T], status, steps,
    sols (the dicts of solve_warm).  It stops at the first step that fails."""
    p = A.shape[0]
    Ap, Bp = (A, B) if plant is None else (plant[0], plant[1])
    cp = plant[2] if plant is not None and len(plant) == 3 and plant[2] is not None else kw.get('offset')
    X = [np.asarray(x0, float)]; U = []; iters = []; codes = []; sols = []
    status = 0
    g, sh = guess, guess_shift
    for t in range(T):
        k = (k0 + t) % p
        r = solve_warm(A, B, H, N, k, X[-1], g, sh, floor, **kw)
        sols.append(r); iters.append(r['iters']); codes.append(r['warm'])
        if r['status'] != 0:
            status = r['status']
            break
        u = r['U'][0]
        U.append(u)
        X.append(callback(t, X[-1], u) if callback is not None else Ap[k] @ X[-1] + Bp[k] @ u + (0.0 if cp is None else cp[k]) + (0.0 if W is None else W[t]))
        g, sh = ({k_: r[k_] for k_ in ('X', 'U', 'Lam', 'Eps', 'Nu', 'NuT')}, 1) if warm else (None, 0)
    return dict(X=np.array(X), U=np.array(U), iters=np.array(iters), warm=np.array(codes), status=status, steps=len(U), sols=sols)


def truth(A, B, H, N, k0, x0, penalty=None, penalty2=None, **kw):
    """(a) cold then (b) of the family's own reference on one step -> (family, its dict): 'quad' solve_quad, 'aff' solve_aff (it is solve_eq with the affine
    vectors), 'soft' solve_soft, 'hard' solve."""
    hardkw = {k: kw.get(k) for k in ('q', 'Pf', 'D', 'd', 'rows')}
    if penalty2 is not None:
        if any(kw.get(k) is not None for k in ('J', 'Tx', 'offset', 'qf', 'trhs')):
            raise ValueError('truth: mpc_qp_quad_reference has no equality rows')
        return 'quad', mqq.solve_quad(A, B, H, N, k0, x0, penalty, penalty2, **hardkw)
    if any(kw.get(k) is not None for k in ('J', 'Tx', 'offset', 'qf', 'trhs')):
        return 'aff', afr.solve_aff(A, B, H, N, k0, x0, penalty, **{k: kw.get(k) for k in ('q', 'Pf', 'D', 'd', 'rows', 'J', 'r', 'erows', 'Tx', 'offset', 'qf', 'trhs')})
    if penalty is not None:
        return 'soft', ms.solve_soft(A, B, H, N, k0, x0, penalty, **hardkw)
    return 'hard', mq.solve(A, B, H, N, k0, x0, **hardkw)


AB = {'hard': mq.ab_disagreement, 'soft': ms.ab_disagreement, 'aff': eqr.ab_disagreement, 'quad': mqq.ab_disagreement}


def against_truth(fam, tr, r):
    """The family's ab_disagreement with the iterate of solve_warm in the place of its method (a)."""
    d = dict(tr)
    d.update(Xa=r['X'], Ua=r['U'], Lama=r['Lam'], Epsa=r['Eps'], Nua=r['Nu'], NuTa=r['NuT'])
    return AB[fam](d)


# ----------------------------------------------------------------------------- the problems (built once per process, never written to)
_CACHE = {}
STEPS = 8
W_STEPS = 12               # steps of the stored disturbance: a loop of T <= W_STEPS steps takes its first T


def _i32(x):
    return None if x is None else np.ascontiguousarray(x, np.int32)


def _hard(case):
    c = case()
    return dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], N=c['N'], k0=c['k0'], opt=dict(q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=_i32(c['rows'])))


def problems():
    """name -> dict A, B, H, X0 [nb,ns,nx], N, k0, opt (the keyword arguments of mpc_qp_batch), loop (those of the loop alone: disturbance), fam, bound (the
    bound of the family's CPU tests for (a) against (b))."""
    if 'problems' in _CACHE:
        return _CACHE['problems']
    from test_mpc_qp_cpu import IPM_VS_POLISH
    out = {}
    for name, case in (('box_nu1', mq.case_box_nu1), ('mixed_small', mq.case_mixed_small), ('single_phase', mq.case_single_phase), ('box_bench', mq.case_box_bench),
                       ('box_nu2', mq.case_box_nu2), ('mixed_bench', mq.case_mixed_bench)):
        out[name] = dict(_hard(case), fam='hard', bound=IPM_VS_POLISH)
    b = ms.batch_of(ms.instances(mq.case_box_nu1, 0.3))
    out['soft'] = dict(A=b['A'], B=b['B'], H=b['H'], X0=b['X0'], N=b['N'], k0=b['k0'], fam='soft', bound=ms.SOFT_IPM_VS_POLISH,
                       opt=dict(q=b['q'], Pf=b['Pf'], D=b['D'], d=b['d'], ndcnt=b['ndcnt'], penalty=b['penalty']))
    b = eqr.batch_of(eqr.case_term_box_nu1())
    out['eq'] = dict(A=b['A'], B=b['B'], H=b['H'], X0=b['X0'], N=b['N'], k0=b['k0'], fam='aff', bound=eqr.EQ_IPM_VS_POLISH,
                     opt={k: b[k] for k in ('q', 'Pf', 'D', 'd', 'ndcnt', 'terminal')})
    b = afr.batch_of(afr.case_aff_qf_box_nu1())
    W = 0.02 * np.random.default_rng(81).standard_normal(b['X0'].shape[:2] + (W_STEPS, b['X0'].shape[2]))
    out['affine'] = dict(A=b['A'], B=b['B'], H=b['H'], X0=b['X0'], N=b['N'], k0=b['k0'], fam='aff', bound=afr.AFF_IPM_VS_POLISH,
                         opt={k: b[k] for k in ('q', 'Pf', 'D', 'd', 'ndcnt', 'qf')}, loop=dict(disturbance=W))
    for name, insts in (('quad_l12', mqq.instances('l12', mq.case_box_nu1, 0.3, 1.0)), ('quad_pure', mqq.instances('pure', mq.case_box_nu1, 1e2))):
        b = mqq.batch_of(insts)
        out[name] = dict(A=b['A'], B=b['B'], H=b['H'], X0=b['X0'], N=b['N'], k0=b['k0'], fam='quad', bound=mqq.QUAD_IPM_VS_POLISH,
                         opt=dict(q=b['q'], Pf=b['Pf'], D=b['D'], d=b['d'], ndcnt=b['ndcnt'], penalty=b['penalty'], penalty2=b['penalty2']))
    for pr in out.values():
        pr.setdefault('loop', {})
        pr['opt'] = {k: v for k, v in pr['opt'].items() if v is not None}
    _CACHE['problems'] = out
    return out


def member_kw(pr, b):
    """The keyword arguments of solve_warm / closed_loop_warm / truth (but W) for member b of a problem."""
    o = pr['opt']
    pick = lambda k: None if o.get(k) is None else o[k][b]
    tx = o.get('terminal')
    kw = dict(q=pick('q'), Pf=pick('Pf'), D=pick('D'), d=pick('d'), rows=pick('ndcnt'), J=pick('J'), r=pick('r'), erows=pick('necnt'),
              Tx=tx if tx is None or isinstance(tx, str) else tx[b], offset=pick('offset'), qf=pick('qf'), trhs=pick('terminal_rhs'), penalty=pick('penalty'),
              penalty2=pick('penalty2'))
    return {k: v for k, v in kw.items() if v is not None}


def loops(name, warm, T=STEPS, floor=WARM_FLOOR, relative=False):
    """closed_loop_warm for every instance of a problem, once per process -> list [nb][ns]."""
    key = ('loops', name, warm, T, floor, relative)
    if key not in _CACHE:
        pr = problems()[name]
        W = pr['loop'].get('disturbance')
        _CACHE[key] = [[closed_loop_warm(pr['A'][b], pr['B'][b], pr['H'][b], pr['N'], pr['k0'], x0, T, warm=warm, floor=floor, relative=relative, W=None if W is None else W[b, s, :T],
                                         **member_kw(pr, b)) for s, x0 in enumerate(pr['X0'][b])] for b in range(pr['A'].shape[0])]
    return _CACHE[key]
