"""Plain-numpy statement of the AFFINE MPC step and of its loop on a plant that is not the model (test infrastructure of test_mpc_qp_affine_cpu.py /
test_gpu_mpc_qp_affine.py on top of mpc_qp_eq_reference, imported and not changed).  To the QP of that module it adds, with k_j = (k0 + j) mod p and
k_N = (k0 + N) mod p,

    x_{j+1} = A_k x_j + B_k u_j + c_k,      the terminal cost  + qf_{k_N}' x_N,      Tx_{k_N} x_N = t_{k_N},

and to the loop the plant  x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t.

`dense_aff` builds the dense problem of mpc_qp_eq_reference.dense_eq and then puts c into b (b[j nx:(j+1) nx] += c_k), t into the last nt entries of re and
qf into c[ix(N)].  `ipm_eq` (method (a)) and `polish_eq` (method (b)) of mpc_qp_eq_reference run on that as they are: the iteration needs no new rule.  In
particular the terminal rows keep their scale max(1, max|x|) in the stop test, and |c|, |t| enter no scale.  The library runs the same iteration stage by
stage (csrc/tmpc_mpc_qp.h, the AFF instantiations).

`shift` restates mpc_qp.about_reference for one problem: a deviation-coordinate problem and a periodic reference -> the absolute-coordinate problem, whose
solution is the deviation solution plus the reference with the same multipliers.

The cases: every value case is feasible with a valid certificate, margin >= MARGIN_MIN and, where it has inequality rows, an active one
(test_mpc_qp_affine_cpu.py checks this on every instance before a GPU sees the case).  The scales that make it so are written at the cases."""
import numpy as np

import mpc_qp_reference as mq
import mpc_qp_soft_reference as sq
import mpc_qp_eq_reference as eqr

# (a) against (b) over every value case below, the scales of mpc_qp_eq_reference.ab_disagreement.  Measured (test_mpc_qp_affine_cpu.py prints every figure
# and asserts the bound); rounded up to one digit.
AFF_IPM_VS_POLISH = 2e-10
# (b) of a shifted case against (b) of its deviation problem plus the reference, same scales; measured and rounded up likewise.
AFF_SHIFT_VS_DEV = 5e-14
# (b) without rows against the condensed dense solve `lq_condensed`, relative to max(1, max|.|); measured and rounded up likewise.
AFF_POLISH_VS_DENSE = 7e-16
MARGIN_MIN = eqr.MARGIN_MIN
T_LOOP = 7


def dense_aff(A, B, H, N, k0, x0, offset=None, qf=None, trhs=None, **kw):
    """mpc_qp_eq_reference.dense_eq (kw: q, Pf, D, d, rows, J, r, erows, Tx) with offset [p,nx], qf [p,nx], trhs [p,nt] (None: zero) put into b, c and re."""
    P = eqr.dense_eq(A, B, H, N, k0, x0, **kw)
    p, nx = A.shape[0], P['nx']
    kN = (k0 + N) % p
    if offset is not None:
        for j in range(N):
            P['b'][j * nx:(j + 1) * nx] += offset[(k0 + j) % p]
    if trhs is not None:
        if not P['nt']:
            raise ValueError('dense_aff: trhs describes the terminal rows, and there are none')
        P['re'][len(P['re']) - P['nt']:] = trhs[kN]
    if qf is not None:
        P['c'][P['ix'](N)] += qf[kN]
    return P


def solve_aff(A, B, H, N, k0, x0, penalty=None, tol=mq.TOL, max_iter=mq.MAX_ITER, offset=None, qf=None, trhs=None, **kw):
    """(a) then (b) on one instance: the dict of mpc_qp_eq_reference.solve_eq."""
    P = dense_aff(A, B, H, N, k0, x0, offset, qf, trhs, **kw)
    cvec = sq.row_penalty(P, penalty, k0) if penalty is not None else np.full(len(P['h']), np.inf)
    a = eqr.ipm_eq(P, cvec, tol, max_iter)
    bb = eqr.polish_eq(P, cvec, sq.states_of(a, cvec) if len(P['h']) else np.zeros(0, int))
    st = bb['state']
    X, U, Lam = mq.unpack(P, bb['v'], bb['lam'])
    Xa, Ua, Lama = mq.unpack(P, a['v'], a['lam'])
    Nu, NuT = eqr.unpack_nu(P, bb['nue']); Nua, NuTa = eqr.unpack_nu(P, a['nue'])
    s0 = P['stage'] == 0
    return dict(a=a, b=bb, X=X, U=U, Lam=Lam, Eps=mq.unpack(P, bb['v'], bb['e'])[2], Nu=Nu, NuT=NuT, Xa=Xa, Ua=Ua, Lama=Lama, Epsa=mq.unpack(P, a['v'], a['e'])[2],
                Nua=Nua, NuTa=NuTa, nact0=int((s0 & (st != sq.INACTIVE)).sum()) if len(st) else 0, nviol0=int((s0 & (st == sq.VIOLATED)).sum()) if len(st) else 0,
                nact_all=int((st != sq.INACTIVE).sum()) if len(st) else 0,
                eres0=eqr.stage_eres(A, k0, X[0], U[0], kw.get('J'), kw.get('r'), kw.get('erows')), P=P, cvec=cvec)


def kkt_check_aff(A, B, H, N, k0, X, U, Lam, Nu, NuT, Eps=None, penalty=None, q=None, Pf=None, D=None, d=None, rows=None, J=None, r=None, erows=None, Tx=None,
                  offset=None, qf=None, trhs=None):
    """mpc_qp_eq_reference.kkt_check_eq for the affine problem: dyn carries c (max|A x + B u + c - x+| / max(1, max|X|)), term carries t
    (max|Tx x_N - t| / max(1, max|X|)), the adjoint recursion starts from pi_N = Pf x_N + qf + Tx' nu_T; the other figures as there."""
    p, nx = A.shape[0], A.shape[1]
    kN = (k0 + N) % p
    dyn = eq = comp = comp_e = stat = gmax = 0.0
    viol, lam_min = -np.inf, np.inf
    xs = max(1.0, np.abs(X).max())
    pi = np.zeros(nx) if Pf is None else ((Pf[kN] + Pf[kN].T) / 2) @ X[N]
    if qf is not None:
        pi = pi + qf[kN]
    term = 0.0
    if Tx is not None:
        T = np.eye(nx) if isinstance(Tx, str) else np.asarray(Tx[kN], float)
        pi = pi + T.T @ NuT
        term = np.abs(T @ X[N] - (0.0 if trhs is None else trhs[kN])).max() / xs
    for j in range(N - 1, -1, -1):
        k = (k0 + j) % p
        z = np.concatenate([X[j], U[j]])
        E = np.concatenate([A[k], B[k]], axis=1)
        dyn = max(dyn, np.abs(E @ z + (0.0 if offset is None else offset[k]) - X[j + 1]).max())
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


def closed_loop_aff(A, B, H, N, k0, x0, T, penalty=None, plant=None, W=None, **kw):
    """The receding-horizon loop on (b) with the plant x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t (plant = (Ap, Bp) or (Ap, Bp, cp), None: the model; a cp left
    out is the model's offset; W [T,nx] or None) -> dict X, U, nact, nviol [steps] (stage 0), hres, eres [steps], status (0, or the status of (a) at the step
    that did not converge), steps (finished), margin, certificate (over the finished steps)."""
    p, nx = A.shape[0], A.shape[1]
    D, d, rows = kw.get('D'), kw.get('d'), kw.get('rows')
    Ap, Bp = (A, B) if plant is None else (plant[0], plant[1])
    cp = plant[2] if plant is not None and len(plant) == 3 and plant[2] is not None else kw.get('offset')
    X = [np.asarray(x0, float)]; U = []; nact = []; nviol = []; hres = []; eres = []; margin = np.inf; cert = True
    status = 0
    for t in range(T):
        k = (k0 + t) % p
        r = solve_aff(A, B, H, N, k, X[-1], penalty, **kw)
        if r['a']['status'] != 0:
            status = r['a']['status']
            break
        u = r['U'][0]
        z = np.concatenate([X[-1], u])
        rk = 0 if D is None else int(D.shape[1] if rows is None else rows[k])
        hres.append((D[k, :rk] @ z - d[k, :rk]).max() if rk else -np.inf)
        eres.append(r['eres0'])
        U.append(u); nact.append(r['nact0']); nviol.append(r['nviol0']); margin = min(margin, r['b']['margin'])
        cert = cert and r['b']['certificate']
        X.append(Ap[k] @ X[-1] + Bp[k] @ u + (0.0 if cp is None else cp[k]) + (0.0 if W is None else W[t]))
    return dict(X=np.array(X), U=np.array(U), nact=np.array(nact), nviol=np.array(nviol), hres=np.array(hres), eres=np.array(eres), status=status, steps=len(U),
                margin=margin, certificate=cert)


def lq_condensed(A, B, H, N, k0, x0, q=None, Pf=None, offset=None, qf=None):
    """The affine LQ problem without rows by a plain dense solve that shares nothing with dense / polish: the states eliminated,
    x_j = Phi_j x_0 + sum_i Gam_{j,i} u_i + g_j, and the normal equations in u -> X [N+1,nx], U [N,mb]."""
    p, nx, mb = A.shape[0], A.shape[1], B.shape[2]
    Phi = [np.eye(nx)]; Gam = [np.zeros((nx, N * mb))]; g = [np.zeros(nx)]
    for j in range(N):
        k = (k0 + j) % p
        G = A[k] @ Gam[-1]
        G[:, j * mb:(j + 1) * mb] += B[k]
        Phi.append(A[k] @ Phi[-1]); Gam.append(G); g.append(A[k] @ g[-1] + (0.0 if offset is None else offset[k]))
    M = np.zeros((N * mb, N * mb)); f = np.zeros(N * mb)
    for j in range(N + 1):
        xa = Phi[j] @ x0 + g[j]                                               # x_j = xa + Gam_j u
        if j < N:
            k = (k0 + j) % p
            Hk = (H[k] + H[k].T) / 2
            S = np.zeros((nx + mb, N * mb)); S[:nx] = Gam[j]; S[nx + np.arange(mb), j * mb + np.arange(mb)] = 1.0
            za = np.concatenate([xa, np.zeros(mb)])
            M += S.T @ Hk @ S; f += S.T @ (Hk @ za + (0.0 if q is None else q[k]))
        else:
            kN = (k0 + N) % p
            Pn = np.zeros((nx, nx)) if Pf is None else (Pf[kN] + Pf[kN].T) / 2
            M += Gam[j].T @ Pn @ Gam[j]; f += Gam[j].T @ (Pn @ xa + (0.0 if qf is None else qf[kN]))
    u = np.linalg.solve(M, -f)
    return np.array([Phi[j] @ x0 + g[j] + Gam[j] @ u for j in range(N + 1)]), u.reshape(N, mb)


def shift(A, B, H, xref, uref, q=None, Pf=None, D=None, d=None, J=None, r=None, Tx=None):
    """One problem (A [p,nx,nx], ...) in deviation coordinates and a periodic reference xref [p,nx], uref [p,mb] -> dict offset, q, d, r, qf, trhs of the
    problem in absolute coordinates (None where the argument is None): what mpc_qp.about_reference states, written out stage by stage."""
    p, nx = A.shape[0], A.shape[1]
    w = np.concatenate([xref, uref], axis=1)
    out = dict(offset=np.array([xref[(k + 1) % p] - A[k] @ xref[k] - B[k] @ uref[k] for k in range(p)]), d=None, r=None, qf=None, trhs=None)
    out['q'] = np.array([(0.0 if q is None else q[k]) - ((H[k] + H[k].T) / 2) @ w[k] for k in range(p)])
    if D is not None:
        out['d'] = np.array([d[k] + D[k] @ w[k] for k in range(p)])
    if J is not None:
        out['r'] = np.array([(0.0 if r is None else r[k]) + J[k] @ w[k] for k in range(p)])
    if Pf is not None:
        out['qf'] = np.array([-((Pf[k] + Pf[k].T) / 2) @ xref[k] for k in range(p)])
    if Tx is not None:
        out['trhs'] = xref.copy() if isinstance(Tx, str) else np.array([Tx[k] @ xref[k] for k in range(p)])
    return out


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def kwargs(c, b=0):
    """The keyword arguments of dense_aff / solve_aff / closed_loop_aff / kkt_check_aff (but penalty) for member b of a case."""
    kw = eqr.kwargs(c, b)
    kw.update({k: None if c.get(k) is None else c[k][b] for k in ('offset', 'qf', 'trhs')})
    return kw


def _shifted(name, base, seed, ref_scale=1.0):
    """base: a case of mpc_qp_eq_reference.  A seeded random periodic reference of order ref_scale, the case in absolute coordinates and what it came from:
    dev (the base), xref [nb,p,nx], uref [nb,p,mb]; X0 is the base's X0 plus xref at phase k0."""
    if name not in _CACHE:
        nb, p, nx, _ = base['A'].shape
        mb = base['B'].shape[3]
        rng = np.random.default_rng(seed)
        xref = ref_scale * rng.standard_normal((nb, p, nx)); uref = ref_scale * rng.standard_normal((nb, p, mb))
        c = dict(base)
        sh = [shift(base['A'][b], base['B'][b], base['H'][b], xref[b], uref[b], **{k: v for k, v in eqr.kwargs(base, b).items() if k not in ('rows', 'erows')})
              for b in range(nb)]
        stack = lambda k: None if sh[0][k] is None else np.array([s[k] for s in sh])
        c.update(name=name, dev=base, xref=xref, uref=uref, X0=base['X0'] + xref[:, base['k0']][:, None], offset=stack('offset'), q=stack('q'), d=stack('d'),
                 r=stack('r'), qf=stack('qf'), trhs=stack('trhs'))
        _CACHE[name] = c
    return _CACHE[name]


def _affine(name, base, seed, x0_scale=1.0, c_scale=0.0, t_scale=0.0, qf_scale=0.0, penalty_f=None, **over):
    """base: a case of mpc_qp_eq_reference (over: entries that replace the base's).  Seeded random offset, terminal right-hand side and qf of the given scales
    (0: None); X0 is x0_scale times the base's; penalty_f: every row soft at penalty_f times the largest multiplier of the hard solutions."""
    if name not in _CACHE:
        nb, p, nx, _ = base['A'].shape
        rng = np.random.default_rng(seed)
        c = dict(base)
        c.update(over)
        nt = 0 if c['Tx'] is None else (nx if isinstance(c['Tx'], str) else c['Tx'].shape[2])
        cc, tt, qq = rng.standard_normal((nb, p, nx)), rng.standard_normal((nb, p, max(nt, 1)))[:, :, :nt], rng.standard_normal((nb, p, nx))
        c.update(name=name, X0=x0_scale * base['X0'], offset=c_scale * cc if c_scale else None, trhs=t_scale * tt if t_scale else None,
                 qf=qf_scale * qq if qf_scale else None, penalty=None, dev=None)
        if penalty_f is not None:
            hard = [[solve_aff(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, **kwargs(c, b)) for x0 in c['X0'][b]] for b in range(nb)]
            lmax = max(h['Lam'].max() for hb in hard for h in hb)
            c['penalty'] = np.full(c['d'].shape, penalty_f * (lmax if lmax > 0 else 1.0))
        _CACHE[name] = c
    return _CACHE[name]


# 1. shifted: the cases of mpc_qp_eq_reference (their X0 scales as there) about a random periodic reference of order 1
def case_shift_term_box_nu1():
    return _shifted('shift_term_box_nu1', eqr.case_term_box_nu1(), 41)


def case_shift_tx_box_nu2():
    return _shifted('shift_tx_box_nu2', eqr.case_tx_box_nu2(), 42)


def case_shift_rows_mixed_small():
    return _shifted('shift_rows_mixed_small_4', eqr.case_rows_mixed_small(4), 43)


def case_shift_rows_mixed_small_N2():
    return _shifted('shift_rows_mixed_small_2', eqr.case_rows_mixed_small(2), 44)


def case_shift_term_p1():
    return _shifted('shift_term_p1', eqr.case_term_p1(), 45)


def case_shift_term_box_bench():
    return _shifted('shift_term_box_bench', eqr.case_term_box_bench(), 46)


def case_shift_soft():
    return _shifted('shift_soft', eqr.case_soft(), 47)


# 2. genuinely affine.  Scales: X0 as in the base case of mpc_qp_eq_reference unless stated; c, t, qf as stated.
def case_aff_term_box_nu2():
    """box_nu2, x_N = t: c of scale 0.2, t of scale 0.1 (at 0.3 / 0.2 two of the four instances cannot reach t inside the input box)."""
    return _affine('aff_term_box_nu2', eqr.case_term_box_nu2(), 51, c_scale=0.2, t_scale=0.1)


def case_aff_term_mixed_small():
    """mixed_small (ragged random rows, q != 0; X0 at 0.3 as in rows_mixed_small), x_N = t: c of scale 0.1, t of scale 0.1."""
    return _affine('aff_term_mixed_small', eqr.case_rows_mixed_small(4), 52, c_scale=0.1, t_scale=0.1, J=None, r=None, erows=None, Tx='constraint')


def case_aff_qf_box_nu1():
    """box_nu1 (N = 5 from phase 2) with Pf = I and qf of scale 0.5, no terminal rows."""
    return _affine('aff_qf_box_nu1', eqr.case_term_box_nu1(), 53, qf_scale=0.5, Tx=None)


def case_aff_tx_soft_box_nu2():
    """box_nu2 with Tx of 2 rows, t of scale 0.3 and every row soft at 0.3 times the largest hard multiplier (some rows violated)."""
    return _affine('aff_tx_soft_box_nu2', eqr.case_tx_box_nu2(), 54, t_scale=0.3, penalty_f=0.3)


def case_aff_bench():
    """The bench stage shape (mixed_bench rows, N = 6) with 2 equality rows per stage, 5 terminal rows: c of scale 0.1, t of scale 0.1."""
    return _affine('aff_bench', eqr.case_rows_mixed_bench(), 55, c_scale=0.1, t_scale=0.1)


def case_aff_edge():
    """nx 40 / nu 24 at N = 2 (the layout edge) with its equality rows, 3 terminal rows: c of scale 0.1, t of scale 0.1."""
    return _affine('aff_edge', eqr.case_edge(), 56, c_scale=0.1, t_scale=0.1)


# 3. no rows at all
def case_aff_no_rows():
    """box_nu2 without D and J: c of scale 0.5, qf of scale 0.5 with Pf = I."""
    return _affine('aff_no_rows', eqr.case_term_box_nu2(), 57, c_scale=0.5, qf_scale=0.5, Tx=None, D=None, d=None, rows=None, ncnt=None)


SHIFT_CASES = [case_shift_term_box_nu1, case_shift_tx_box_nu2, case_shift_rows_mixed_small, case_shift_rows_mixed_small_N2, case_shift_term_p1,
               case_shift_term_box_bench, case_shift_soft]
AFFINE_CASES = [case_aff_term_box_nu2, case_aff_term_mixed_small, case_aff_qf_box_nu1, case_aff_tx_soft_box_nu2, case_aff_bench, case_aff_edge]
VALUE_CASES = SHIFT_CASES + AFFINE_CASES


def solve_case(c):
    """Every instance of a case through (a) and (b), once per process -> list [nb][ns] of the dicts of solve_aff."""
    key = ('solved', c['name'])
    if key not in _CACHE:
        _CACHE[key] = [[solve_aff(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0, None if c['penalty'] is None else c['penalty'][b], **kwargs(c, b))
                        for x0 in c['X0'][b]] for b in range(c['A'].shape[0])]
    return _CACHE[key]


def batch_of(c):
    """A case -> the batch arguments: the dict of mpc_qp_eq_reference.batch_of with offset, qf, terminal_rhs."""
    out = eqr.batch_of(c)
    out.update(offset=c['offset'], qf=c['qf'], terminal_rhs=c['trhs'])
    return out


def shifted_solution(c, r_dev, b=0):
    """The solution of a shifted case predicted from the solution r_dev of its deviation problem: X + xref at the phases, U + uref."""
    p = c['A'].shape[1]
    N, k0 = c['N'], c['k0']
    ph = (k0 + np.arange(N + 1)) % p
    return r_dev['X'] + c['xref'][b][ph], r_dev['U'] + c['uref'][b][ph[:N]]


# 4. the loops, T = T_LOOP
def loop_shift():
    """(i) shift_term_box_nu1 run in absolute coordinates."""
    return case_shift_term_box_nu1()


def loop_plant():
    """(ii) term_box_nu2 with plant = (A + dA, B), dA of scale 0.05, and a seeded W of scale 0.02 -> (case, plant (Ap, Bp) [nb,p,..], W [nb,ns,T,nx])."""
    c = _affine('loop_plant', eqr.case_term_box_nu2(), 61)
    if 'loop_plant_data' not in _CACHE:
        rng = np.random.default_rng(62)
        _CACHE['loop_plant_data'] = ((c['A'] + 0.05 * rng.standard_normal(c['A'].shape), c['B'].copy()),
                                     0.02 * rng.standard_normal(c['X0'].shape[:2] + (T_LOOP, c['X0'].shape[2])))
    return (c,) + _CACHE['loop_plant_data']


X1_BOUND = 0.1
PUSH_PENALTY = 50.0


def loop_push():
    """(iii) the box_nu1 model (p 3 / nx 3 / nu 1, N = 5 from phase 2) with the hard rows +-x_1 <= X1_BOUND on the first state and no others, started inside
    (X0: the base's first state scaled to max|x| = 0.05), and a disturbance that pushes x_1 outside: the undisturbed loop is run here, and W_{t* - 1} moves
    the first state of step t* = 3 to 0.3, so that the QP of step t* starts outside its bound -> (case with the hard rows, W [1,1,T,nx], t*).  With hard
    rows that QP is infeasible (its row of stage 0 is on x_0 alone); with the penalty PUSH_PENALTY on both rows the loop goes on."""
    if 'loop_push' not in _CACHE:
        base = mq.case_box_nu1()
        nb, p, nx, _ = base['A'].shape
        n = nx + base['B'].shape[3]
        D = np.zeros((1, p, 2, n)); D[:, :, 0, 0] = 1.0; D[:, :, 1, 0] = -1.0
        c = dict(A=base['A'][:1], B=base['B'][:1], H=base['H'][:1], Pf=base['Pf'][:1], q=None, D=D, d=np.full((1, p, 2), X1_BOUND), rows=np.full((1, p), 2), ncnt=None,
                 J=None, r=None, erows=None, Tx=None, penalty=None, offset=None, qf=None, trhs=None, N=base['N'], k0=base['k0'], name='loop_push', dev=None)
        x0 = 0.05 * base['X0'][0, 0] / np.abs(base['X0'][0, 0]).max()
        c['X0'] = x0[None, None]
        free = closed_loop_aff(c['A'][0], c['B'][0], c['H'][0], c['N'], c['k0'], x0, T_LOOP, **kwargs(c))
        ts = 3                                                               # the state that step 3 starts from is pushed: t* = 3 >= 2
        W = np.zeros((1, 1, T_LOOP, nx))
        W[0, 0, ts - 1, 0] = 0.3 - free['X'][ts, 0]
        _CACHE['loop_push'] = (c, W, ts)
    return _CACHE['loop_push']


# 5. infeasible: N mb = 2 < nt = 3 with t != 0 (the box_nu1 model at N = 2, x_N = t)
def infeasible_instance():
    c = mq.case_box_nu1()
    t = np.random.default_rng(71).standard_normal((3, 3))
    return dict(A=c['A'][:1], B=c['B'][:1], H=c['H'][:1], Pf=c['Pf'][:1], X0=c['X0'][:1, :1], N=2, k0=2, terminal='constraint', terminal_rhs=t[None])
