"""Plain-numpy statement of the local gain of a solved MPC step (test infrastructure of test_mpc_qp_gain_cpu.py / test_gpu_mpc_qp_gain*.py; nothing under
tunempc_amd/ imports it).  At a strictly complementary solution the QP of mpc_qp_reference is locally affine in x_0: u_0(x_0 + dx) = u_0 - K_0 dx.

`classify` states the rule (csrc/tmpc_mpc_qp_gain.h mirrors it).  With g = d_i - D_i z_j, per row (j, i) of the horizon:
    hard row (c = inf)                 s = g                                 1 if lam > s, else 0
    pure quadratic (c = 0, Z > 0)      s = g + lam / Z                       2 if lam > s, else 0
    0 < c < inf                        s = g + e, nu = c + Z e - lam         0 if not lam > s; else violated (e > nu): 2 if Z > 0, 0 if Z = 0; not violated: 1
    rows beyond the stage's count                                            0
0 free: the row drops out; 1 equality: D_i dz_j = 0; 2 quadratic: the stage Hessian gains Z_i D_i' D_i.  strict = min over the pairs (lam, s) and, on
two-pair rows, (e, nu) of |a - b| / max(|a|, |b|) (0 where both vanish; 1 when there is no pair).

Method (a), `gain`: the recursion of lqr_horizon_reference.horizon_lqr on the per-instance expanded data (`expand`): stage j takes A, B, H of phase
(k0 + j) mod p, the rows [J_k; class-1 rows of D_k] as its equality rows and the class-2 terms in H.  Terminal rows Tx start the same recursion from
Hn_N = the orthonormalised rows of Tx (`_pass`, the loop of horizon_lqr with a given start).
Method (b), `fd_gain`: the central difference, at h = 1e-4, of the polished active-set solution (mpc_qp_quad_reference.polish_quad, which is polish /
polish_soft on hard / soft rows): that solution is exactly affine while the set holds, so the difference carries rounding only.  Taken along the columns
of Pz_0 = I - Hn_0' Hn_0, the directions in which the active set can be kept.
Method (c), `kkt_gain`: lqr_horizon_reference.kkt_first_input, one dense null-space solve of the expanded equality-constrained problem."""
import numpy as np

import lqr_ctg_reference as lc
import lqr_horizon_reference as lh
import lqr_rows_reference as lrr
import mpc_qp_reference as mq
import mpc_qp_quad_reference as mqq

FD_STEP = 1e-4
# (a) against (b) times Pz_0, K_0 and the open-loop sensitivities, relative to max(1, max|.|) of (b): the worst instance of each case as test_mpc_qp_gain_cpu.py
# measures it (it prints every figure and asserts ten times these).  In every run the active set is unchanged at +-h, strict = 1.000000 and the polish
# certificate holds.
AB_MEASURED = {'case_box_nu1': 4.4e-12, 'case_box_nu2': 2.3e-12, 'case_mixed_small': 2.1e-11, 'case_single_phase': 3.1e-12, 'case_box_bench': 7.0e-11,
               'case_mixed_bench': 4.4e-10, 'case_state_box': 5.9e-11}
KKT_FLOOR = 1e-13


def ab_bound(case):
    return 10 * AB_MEASURED[case.__name__]


def _pair(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def classify(N, k0, X, U, Lam, Eps, D, d, rows=None, penalty=None, penalty2=None):
    """One instance: X [N+1,nx], U [N,mb], Lam, Eps [N,nd] (Eps None: zero), D [p,nd,n], d [p,nd], rows [p] or None, penalty, penalty2 [p,nd] or None ->
    (cls int [N,nd], strict)."""
    p, nd = D.shape[0], D.shape[1]
    cls = np.zeros((N, nd), int)
    strict = np.inf
    for j in range(N):
        k = (k0 + j) % p
        z = np.concatenate([X[j], U[j]])
        for i in range(nd if rows is None else int(rows[k])):
            g = d[k, i] - D[k, i] @ z
            lam = Lam[j, i]
            e = 0.0 if Eps is None else Eps[j, i]
            c = np.inf if penalty is None else penalty[k, i]
            Z = 0.0 if penalty2 is None else penalty2[k, i]
            if c == np.inf:
                strict = min(strict, _pair(lam, g))
                cls[j, i] = 1 if lam > g else 0
            elif c == 0:
                s = g + lam / Z if Z > 0 else g
                strict = min(strict, _pair(lam, s))
                cls[j, i] = 2 if lam > s and Z > 0 else 0
            else:
                s, nu = g + e, c + Z * e - lam
                strict = min(strict, _pair(lam, s), _pair(e, nu))
                if lam > s:
                    cls[j, i] = (2 if Z > 0 else 0) if e > nu else 1
    return cls, (strict if np.isfinite(strict) else 1.0)


def expand(A, B, H, N, k0, cls, D=None, penalty2=None, Pf=None, J=None, erows=None):
    """The per-instance expanded problem of period N: dict A [N,nx,nx], B, H [N,n,n] (symmetric part, class-2 terms added in ascending i), J [N,nr,n] (the first
    erows_k rows of J_k, then the class-1 rows of D_k in ascending i), rows [N], Pf [N,nx,nx] (Pf[(k0 + N) mod p] at every phase) or None."""
    p, nx = A.shape[0], A.shape[1]
    n = nx + B.shape[2]
    ks = [(k0 + j) % p for j in range(N)]
    He = np.array([(H[k] + H[k].T) / 2 for k in ks])
    stacks = []
    for j, k in enumerate(ks):
        st = [] if J is None else [J[k, i] for i in range(J.shape[1] if erows is None else int(erows[k]))]
        if D is not None:
            for i in range(D.shape[1]):
                if cls[j, i] == 1:
                    st.append(D[k, i])
                elif cls[j, i] == 2:
                    He[j] = He[j] + penalty2[k, i] * np.outer(D[k, i], D[k, i])
        stacks.append(st)
    nr = max(len(s) for s in stacks)
    Je = np.zeros((N, nr, n))
    for j, s in enumerate(stacks):
        if s:
            Je[j, :len(s)] = np.array(s)
    Pn = None
    if Pf is not None:
        Pn = (Pf[(k0 + N) % p] + Pf[(k0 + N) % p].T) / 2
    return dict(A=np.array([A[k] for k in ks]), B=np.array([B[k] for k in ks]), H=He, J=Je if nr else None, rows=np.array([len(s) for s in stacks]),
                Pf=None if Pn is None else np.array([Pn] * N))


def _pass(E, N, Hn, rank_tol):
    """The loop of lqr_horizon_reference.horizon_lqr on expanded data E from a given Hn_N [c,nx] -> its dict."""
    nx, mb = E['A'].shape[1], E['B'].shape[2]
    Pi = np.zeros((nx, nx)) if E['Pf'] is None else np.array(E['Pf'][0])
    K = np.zeros((N, mb, nx)); cnt = np.zeros(N, dtype=int)
    feas = 0.0
    for j in range(N - 1, -1, -1):
        Ej = np.concatenate([E['A'][j], E['B'][j]], axis=1)
        Hb = E['H'][j] + Ej.T @ Pi @ Ej
        Jj = np.zeros((0, nx + mb)) if E['J'] is None else E['J'][j, :int(E['rows'][j])]
        Cf = np.concatenate([Jj, Hn @ Ej], axis=0)
        Jt, Hk = lc.split(Cf, nx, rank_tol)
        cnt[j] = Hk.shape[0]
        if Hk.shape[0] >= nx:
            return dict(infeasible=True, stage=j, cnt=cnt)
        Kk, _, Pk = lrr.stage(Hb, Jt if Jt.shape[0] else None, nx)
        Pz = np.eye(nx) - Hk.T @ Hk
        K[j] = Kk @ Pz
        if Cf.shape[0]:
            feas = max(feas, np.abs((Cf[:, :nx] - Cf[:, nx:] @ K[j]) @ Pz).max())
        Pi = Pz @ Pk @ Pz
        Pi = (Pi + Pi.T) / 2
        Hn = Hk
    return dict(infeasible=False, K=K, cnt=cnt, K0=K[0], Pi0=Pi, Hn0=Hn, Pz0=np.eye(nx) - Hn.T @ Hn, feas=feas)


def gain(A, B, H, N, k0, cls, D=None, penalty2=None, Pf=None, J=None, erows=None, terminal=None, rank_tol=1e-9):
    """Method (a) on one instance.  terminal: None, 'constraint' or Tx [p,nt,nx] -> the dict of lqr_horizon_reference.horizon_lqr, with E (the expanded data)."""
    E = expand(A, B, H, N, k0, cls, D, penalty2, Pf, J, erows)
    if terminal is None or isinstance(terminal, str):
        r = lh.horizon_lqr(E['A'], E['B'], E['H'], E['J'], E['rows'], N, 0, 'constraint' if terminal is not None else 'cost', E['Pf'], rank_tol)
    else:
        p, nx, mb = A.shape[0], A.shape[1], B.shape[2]
        Tx = terminal[(k0 + N) % p]
        _, Hn = lc.split(np.concatenate([Tx, np.zeros((Tx.shape[0], mb))], axis=1), nx, rank_tol)
        r = _pass(E, N, Hn, rank_tol)
    r['E'] = E
    return r


def sensitivities(E, r, N):
    """The open-loop sensitivities of a pass: dX [N+1,nx,nx], dU [N,mb,nx] with Phi_0 = Pz_0, dU_j = -K_j Phi_j, Phi_{j+1} = A Phi_j + B dU_j."""
    dX = [r['Pz0']]; dU = []
    for j in range(N):
        dU.append(-r['K'][j] @ dX[-1])
        dX.append(E['A'][j] @ dX[-1] + E['B'][j] @ dU[-1])
    return np.array(dX), np.array(dU)


def kkt_gain(r, N, terminal=None):
    """Method (c) on the expanded data of a pass r of `gain` (terminal None or 'constraint') -> max|u_0 of the dense solve + K_0 x_0| / max(1, max|K_0|) over a
    basis of null(Hn_0)."""
    E = r['E']
    Z0, U0 = lh.kkt_first_input(E['A'], E['B'], E['H'], E['J'], E['rows'], N, 0, 'constraint' if terminal is not None else 'cost', E['Pf'], r['Hn0'])
    return np.abs(U0 + r['K0'] @ Z0).max() / max(1.0, np.abs(r['K0']).max())


def solve_instance(i):
    """An instance dict of mpc_qp_soft_reference.instances / mpc_qp_quad_reference.instances (penalty / penalty2 optional: hard rows) through the interior-point
    reference and its polish -> the dict of mpc_qp_quad_reference.finish_quad."""
    kw = i['kw']
    nd = kw['D'].shape[1]
    pen = i.get('penalty', np.full((i['A'].shape[0], nd), np.inf))
    pen2 = i.get('penalty2', np.zeros((i['A'].shape[0], nd)))
    return mqq.solve_quad(i['A'], i['B'], i['H'], i['N'], i['k0'], i['x0'], pen, pen2, **kw)


def fd_gain(i, r, Pz0, h=FD_STEP):
    """Method (b): r = solve_instance(i).  Central differences of the polished solution with the state pattern of r along the columns of Pz0 ->
    dict K0 [mb,nx] (= K_0 Pz_0), dX [N+1,nx,nx], dU [N,mb,nx], certificate (the polish certificate held at every x_0 +- h Pz_0 e_c: the active set is unchanged)."""
    nx = i['A'].shape[1]
    N = i['N']
    cert = True
    cols = []
    for c in range(nx):
        side = []
        for sgn in (1.0, -1.0):
            P = mq.dense(i['A'], i['B'], i['H'], N, i['k0'], i['x0'] + sgn * h * Pz0[:, c], **i['kw'])
            b = mqq.polish_quad(P, r['cvec'], r['zvec'], r['state'])
            cert = cert and b['certificate'] and np.array_equal(b['state'], r['state'])
            X, U, _ = mq.unpack(P, b['v'])
            side.append((X, U))
        cols.append(((side[0][0] - side[1][0]) / (2 * h), (side[0][1] - side[1][1]) / (2 * h)))
    dX = np.stack([c[0] for c in cols], axis=2); dU = np.stack([c[1] for c in cols], axis=2)
    return dict(K0=-dU[0], dX=dX, dU=dU, certificate=bool(cert))


def gain_of_instance(i, r, cls=None, rank_tol=1e-9):
    """Method (a) at the polished solution r of instance i (cls None: by the rule) -> (dict of `gain`, cls, strict)."""
    kw = i['kw']
    pen, pen2 = i.get('penalty'), i.get('penalty2')
    c, strict = classify(i['N'], i['k0'], r['X'], r['U'], r['Lam'], r['Eps'], kw['D'], kw['d'], kw['rows'], pen, pen2)
    if cls is None:
        cls = c
    return gain(i['A'], i['B'], i['H'], i['N'], i['k0'], cls, kw['D'], pen2, kw['Pf'], rank_tol=rank_tol), cls, strict


def rel(x, y):
    """max|x - y| / max(1, max|y|)."""
    return float(np.abs(x - y).max() / max(1.0, np.abs(y).max())) if np.size(y) else 0.0


# ----------------------------------------------------------------------------- the cases (built once per process, never written to)
_CACHE = {}


def hard_instances(case):
    """Every (member, state) of a case of mpc_qp_reference as an instance dict (hard rows)."""
    key = ('hard', case.__name__)
    if key not in _CACHE:
        c = case()
        _CACHE[key] = [dict(A=c['A'][b], B=c['B'][b], H=c['H'][b], N=c['N'], k0=c['k0'], x0=x0, kw=mq.kwargs(c, b))
                       for b in range(c['A'].shape[0]) for x0 in c['X0'][b]]
    return _CACHE[key]


def case_state_box():
    """The p 3 / nx 3 / nu 2 base of lqr_horizon_reference.case_ragged_rows, N = 4 from phase 1, Pf = I, rows +-u <= 2 and +-x_1 <= 0.2 at every stage,
    X0 = default_rng(32).standard_normal((1, 4, 3)) with the first component replaced by 0.1 sign(.): active state rows give cnt = [0, 1, 1, 0] and two active
    rows at a stage of two inputs.  Holds both sides of the certificate: Hc (the tracking side, `H` of the solves) and H, P of the base."""
    if 'state_box' not in _CACHE:
        base = lh.case_ragged_rows()
        A, B = base['A'], base['B']
        nb, p, nx, _ = A.shape
        mb = B.shape[3]
        n = nx + mb
        D = np.zeros((nb, p, 2 * mb + 2, n))
        D[:, :, :mb, nx:] = np.eye(mb); D[:, :, mb:2 * mb, nx:] = -np.eye(mb)
        D[:, :, 2 * mb, 0] = 1.0; D[:, :, 2 * mb + 1, 0] = -1.0
        d = np.full((nb, p, 2 * mb + 2), 2.0); d[:, :, 2 * mb:] = 0.2
        X0 = np.random.default_rng(32).standard_normal((1, 4, 3))
        X0[..., 0] = 0.1 * np.sign(X0[..., 0])
        _CACHE['state_box'] = dict(A=A, B=B, H=base['Hc'], Hc=base['Hc'], Hecon=base['H'], P=base['P'],
                                   Pf=np.ascontiguousarray(np.broadcast_to(np.eye(nx), (nb, p, nx, nx))), X0=X0, N=4, k0=1, q=None, ncnt=None, D=D, d=d,
                                   rows=np.full((nb, p), 2 * mb + 2))
    return _CACHE['state_box']


def solved(insts_key, insts):
    """solve_instance over a list of instances, once per process."""
    key = ('solved', insts_key)
    if key not in _CACHE:
        _CACHE[key] = [solve_instance(i) for i in insts]
    return _CACHE[key]


def kkt_disagreement(case):
    """The worst disagreement of methods (a) and (c) over the instances of a hard-row case, at the polished solutions (once per process)."""
    key = ('kkt', case.__name__)
    if key not in _CACHE:
        insts = hard_instances(case)
        _CACHE[key] = max(kkt_gain(gain_of_instance(i, r)[0], i['N']) for i, r in zip(insts, solved(case.__name__, insts)))
    return _CACHE[key]


def batch_of_case(c):
    """A case dict of mpc_qp_reference (or case_state_box) -> the batch arguments of mpc_qp_eq_reference.batch_of (no equality rows, no terminal rows)."""
    return dict(A=c['A'], B=c['B'], H=c['H'], X0=c['X0'], q=c['q'], Pf=c['Pf'], D=c['D'], d=c['d'], ndcnt=None if c['rows'] is None else
                np.ascontiguousarray(c['rows'], np.int32), penalty=None, J=None, r=None, necnt=None, terminal=None, N=c['N'], k0=c['k0'])


def reference_of_batch(bt, sol, cls=None, rank_tol=1e-9):
    """Method (a) at the solutions `sol` (dict of numpy X, U, lam, eps as mpc_qp_batch returns them) of a batch dict (keys of batch_of_case, optionally
    penalty2) -> list [nb][ns] of (dict of `gain`, cls, strict); cls [nb,ns,N,nd] replaces the rule."""
    out = []
    nb, ns = bt['X0'].shape[:2]
    pick = lambda k, b: None if bt.get(k) is None else bt[k][b]
    for b in range(nb):
        row = []
        for s in range(ns):
            if bt['D'] is None:
                c, strict = np.zeros((bt['N'], 0), int), 1.0
            else:
                eps = sol.get('eps')
                c, strict = classify(bt['N'], bt['k0'], sol['X'][b, s], sol['U'][b, s], sol['lam'][b, s], None if eps is None else eps[b, s], bt['D'][b], bt['d'][b],
                                     pick('ndcnt', b), pick('penalty', b), pick('penalty2', b))
            if cls is not None:
                c = cls[b, s]
            term = bt['terminal'] if bt['terminal'] is None or isinstance(bt['terminal'], str) else bt['terminal'][b]
            row.append((gain(bt['A'][b], bt['B'][b], bt['H'][b], bt['N'], bt['k0'], c, pick('D', b), pick('penalty2', b), pick('Pf', b), pick('J', b),
                             pick('necnt', b), term, rank_tol), c, strict))
        out.append(row)
    return out


# ----------------------------------------------------------------------------- equality rows and terminal rows: method (b) on mpc_qp_eq_reference
# (a) against (b) times Pz_0 (K_0 only) on the cases with equality rows J and terminal rows, worst instance per case as test_mpc_qp_gain_cpu.py measures it
# (asserted at ten times these).  The (b) side is the polished solution of mpc_qp_eq_reference: it shares nothing with `_pass`.
AB_EQ_MEASURED = {'case_term_box_nu2': 2.3e-12, 'case_tx_box_nu2': 2.3e-12, 'case_rows_mixed_small': 2.0e-11}


def gain_of_eq_instance(c, b, s, r, rank_tol=1e-9):
    """Method (a) at the polished solution r = mpc_qp_eq_reference.solve_case(c)[b][s] of a case of mpc_qp_eq_reference (hard rows) -> (dict of `gain`, cls, strict)."""
    pick = lambda k: None if c[k] is None else c[k][b]
    cls, strict = (np.zeros((c['N'], 0), int), 1.0) if c['D'] is None else classify(c['N'], c['k0'], r['X'], r['U'], r['Lam'], None, c['D'][b], c['d'][b], pick('rows'))
    term = c['Tx'] if c['Tx'] is None or isinstance(c['Tx'], str) else c['Tx'][b]
    return gain(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], cls, pick('D'), None, c['Pf'][b], pick('J'), pick('erows'), term, rank_tol), cls, strict


def fd_gain_eq(c, b, s, r, Pz0, h=FD_STEP):
    """Method (b) with equality and terminal rows: central differences of mpc_qp_eq_reference.polish_eq with the state pattern of r along the columns of Pz0 ->
    dict K0 (= K_0 Pz_0), certificate (polish_eq's, at every x_0 +- h Pz_0 e_c, with an unchanged pattern)."""
    import mpc_qp_eq_reference as eqr
    kw = eqr.kwargs(c, b)
    x0 = c['X0'][b, s]
    st = r['b']['state']
    cert, cols = True, []
    for q in range(len(x0)):
        side = []
        for sgn in (1.0, -1.0):
            P = eqr.dense_eq(c['A'][b], c['B'][b], c['H'][b], c['N'], c['k0'], x0 + sgn * h * Pz0[:, q], **kw)
            bb = eqr.polish_eq(P, None, st)
            cert = cert and bb['certificate'] and np.array_equal(bb['state'], st)
            side.append(mq.unpack(P, bb['v'])[1][0])
        cols.append((side[0] - side[1]) / (2 * h))
    return dict(K0=-np.stack(cols, axis=1), certificate=bool(cert))


# ----------------------------------------------------------------------------- (a) against (c), per instance
# What test_mpc_qp_gain_cpu.py measures per instance (it prints every figure and asserts that none exceeds ten times its figure here): at the active set of the rule, and with every row
# free (one figure per case: without rows the pass does not depend on the instance).  The GPU tests hold two GPU paths of one stage to ten times the figure of
# the same instance, floor KKT_FLOOR.
KKT_MEASURED = {'case_box_nu2': [2.8e-16, 2.6e-16, 2.6e-16, 2.8e-16], 'case_state_box': [3.2e-15, 3.5e-15, 7.8e-16, 3.2e-15],
                'case_box_bench': [6.2e-16, 6.3e-16, 6.8e-16]}
KKT_FREE_MEASURED = {'case_box_nu2': 2.8e-16, 'case_state_box': 7.8e-16, 'case_box_bench': 2.6e-16}


def kkt_instances(case):
    """(a) against (c) per instance of a hard-row case at the polished solutions (once per process) -> list."""
    key = ('kkt_inst', case.__name__)
    if key not in _CACHE:
        insts = hard_instances(case)
        _CACHE[key] = [kkt_gain(gain_of_instance(i, r)[0], i['N']) for i, r in zip(insts, solved(case.__name__, insts))]
    return _CACHE[key]


def kkt_free(case):
    """(a) against (c) with every row free."""
    key = ('kkt_free', case.__name__)
    if key not in _CACHE:
        i = hard_instances(case)[0]
        nd = i['kw']['D'].shape[1]
        _CACHE[key] = kkt_gain(gain(i['A'], i['B'], i['H'], i['N'], i['k0'], np.zeros((i['N'], nd), int), i['kw']['D'], None, i['kw']['Pf']), i['N'])
    return _CACHE[key]


def two_paths_bound(case, s=None):
    """Ten times the stored (a)-against-(c) figure of instance s of the case (s None: every row free), floor KKT_FLOOR."""
    return max(10 * (KKT_FREE_MEASURED[case.__name__] if s is None else KKT_MEASURED[case.__name__][s]), KKT_FLOOR)
