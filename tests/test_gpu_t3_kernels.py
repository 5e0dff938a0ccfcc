"""Kernel-level check of the Step 3 kernels (tunempc_amd/csrc/tmpc_t3.h): k_t3_init, k_t3_pre, k_t3_schur<false / true>, k_t3_cross, k_t3_rhs, k_t3_gather, k_t3_dir,
k_t3_steps, k_t3_update -- the rows of theta_k >= 0 and of the norm cone (t_k; w c o theta_k), the only second-order cone the project treats natively -- at iterates
the SOLVER reached.  A call runs iterations 1 .. K-1 as always and stops inside iteration K at one of four points (TMPC_DEBUG_FLAG_STOP_ASSEMBLED +
tmpc_debug_set_stop_point):
    s0  the assembled system and the pass-1 right-hand sides        s1  after pass 1 and k_ctrl_b        s2  pass 2 complete, before k_ctrl_c        s3  iteration K complete
one device call per point, all on one handle with chunk = batch and lanes = 1 (tmpc_debug_get_array reads lane 0; codes 54 .. 69 are the Step 3 state).

Every layer is compared with tests/t3_reference.py (numpy, np.longdouble) evaluated on that layer's OWN device inputs: |device - reference| <= 4 gamma_m * bound
entrywise, bound and m carried through the reference's arithmetic (its docstring derives the rules; what passes through 1 / sqrt(det u) gets the conditioning
kappa(u) of the cone point from them).  Exceptions: the step length into the cone is accepted by the residual of its root (SOC_ROOT_FACTOR, section c) and against
bisection; the block solve has no rounding bound, so the stage-local rows of the Newton equations are held against a dense fp64 LAPACK solve of the system
assembled at s0 (NEWTON_RESIDUAL_FACTOR of tests/test_gpu_step_kernels.py).  Cases: tests/t3_kernel_cases.py.

Not covered here: a chord step's local Newton rows (its system is not in the workspace: D holds the factor of an earlier iterate), the right-hand side rows of pass 2
other than through the Newton rows (the solve overwrites them), the double-double path and the un-scaling of T_k (k_final: tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import phi_reference as ph
import schur_reference as sr
import t3_reference as t3
from t3_kernel_cases import (CENTER_CASES, LARGE_CASES, MAIN_CASES, P2, SMALL_CASES, make_problem, solved_members, stage_layout)
from step_kernel_cases import (I_CHORD, I_NSHIFT, I_PHASE, I_REG, I_SHIFT0, IS, NPART, P_AD, P_AP, P_BAA, P_BTA, P_BTT, P_CORR0, P_DALPHA, P_DTAU, P_RD0, P_S0, P_SIGMU,
                               P_X0, PH_DONE, PH_MAIN, PS, Q_DXDS, Q_DXS, Q_HBG, Q_TRT2, Q_XDS, TRACE_LEN, TRACE_W, eig_thresholds)
from test_gpu_schur_assembly import _inside
from test_gpu_step_kernels import NEWTON_RESIDUAL_FACTOR

pytestmark = pytest.mark.gpu

LD = sr.LD
EPS = sr.EPS
FLAG_STOP_ASSEMBLED, FLAG_GENERIC_STAGE, FLAG_GENERIC_ROWS = 8, 64, 128
STOPS = (('s0', 0), ('s1', 1), ('s2', 2), ('s3', 3))
P_S, P_SBETA, Q_XS, Q_RPHI2, Q_NCONE = 9, 10, 0, 24, 25           # csrc/tmpc_common.h
AEL = 32
CODES = dict(Ddiag=2, D=3, part=4, O=5, W3=7, U=8, X1=9, X2=10, S1=11, S2=12, P=13, V=14, Hb=15, S1i=16, S2i=17, T1=20, T2=21, Z=25, prob=26, trace=27,
             dP=28, dX1=29, dX2=30, dS1=31, dS2=32, Wm=39, eigmin=40, TU=41)
ROW_CODES = dict(psm=0, pvec=1, G=42, asum=52)
ARROW_CODES = dict(at=44, adt=45, aX=46)
T3_M = dict(th=54, z=55, dth=56, dz=57, cth=58)
T3_M1 = dict(x=59, dx=60, cq=61, g=62, v=63, lam=64)
T3_1 = dict(t=65, dt=66, beta=67)
T3_NN = dict(t3psi=68, t3phi=69)
# The step length into the cone (soc_step_eig) is a root of det(u + th du) = 0; a computed root th is accepted when |det(u + th du)| <= C eps
# (|u0 + th du0|^2 + |u1 + th du1|^2) in longdouble, C taken from the fp64 numpy restatement of the routine (t3_reference.soc_step_eig64) times SOC_ROOT_FACTOR = 10
# for the kernel's wave-order sums and fused multiply-adds: the larger of (i) the residual the restatement leaves on the SAME pair and (ii) the worst residual it
# leaves on the edge pairs of section c AT THE SAME LENGTH m1 (_restatement_floor: 121.75 eps at m1 = 2, where an exit lies next to the apex, 4 .. 5 eps at m1 = 64 ..
# 529: profiles/t3_kernel_residuals.txt).  (ii) keeps the tolerance from collapsing to nothing where the restatement happens to hit the root exactly; (i) is needed
# where the ray leaves next to the apex of the cone: the two roots meet there and the residual of any fp64 th grows without bound.  (iii) The routine returns
# eig = -1 / th and the test inverts it again: two roundings, so even the exact root comes back moved by up to 2 eps relative, which next to the apex
# (|u + th du| small against |th du|) is many eps of residual: |2 (bq + a th) th| 2 eps relative to the same scale, from the longdouble root of the bisection.
# One solver-reached pair needs it (n = 3, K = 1, pass 2: the kernel's root is 7 eps from the exact one and leaves 99.6 eps where (i), (ii) allow 28.6).
SOC_ROOT_FACTOR = 10.0
_FLOOR = {}
PARAMS = MAIN_CASES + CENTER_CASES
_RUNS = {}


def _id(prm):
    (nb, p, nx, mb, ng, nc, ncnt, rho), k, generic = prm
    return f'nb{nb}-p{p}-nx{nx}-mb{mb}-ng{ng}-nc{nc}-rho{rho:g}-' + (f'K{k}' if isinstance(k, int) else k) + ('-generic' if generic else '')


def dims(case, room=None):
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    n = nx + mb; d = nx * (nx + 1) // 2; m = n * (n + 1) // 2
    nr = ng + nc
    nzs = nr + (2 if (ncnt is not None and rho > 0.0) else 0)
    rng_, rnc = (ng, nc) if room is None else room
    return dict(nb=nb, p=p, nx=nx, mb=mb, n=n, d=d, m=m, ng=ng, nc=nc, nr=nr, nzs=nzs, oT=d + nzs, dp=(d + nzs + m + 1 + 15) // 16 * 16, arrows=nzs > nr, rows=nr > 0,
                room=(rng_, rnc))


def _snapshot(h, dm):
    nb, p, nx, n, dp, nr, nzs, m = (dm[k] for k in ('nb', 'p', 'nx', 'n', 'dp', 'nr', 'nzs', 'm'))
    shp = dict(Ddiag=(p, dp), D=(p, dp, dp), O=(p, dp, dp), part=(p, NPART), W3=(p, dp, 3), U=(p, dp, 2), TU=(p, dp, 2), Z=(p, dp), P=(p, nx, nx), dP=(p, nx, nx),
               V=(p, nx, n), prob=(PS,), trace=(TRACE_LEN, TRACE_W), Wm=(p, 4, n, n), eigmin=(p, 4), psm=(p, nzs * nzs + 6 * nzs), pvec=(p, 2, nr, 2 * n + 2 * nx),
               G=(p, nr, n), asum=(p, 5), at=(p, 2), adt=(p, 2), aX=(p, 2, AEL, AEL))
    codes = dict(CODES)
    if dm['rows']:
        codes.update(ROW_CODES)
    if dm['arrows']:
        codes.update(ARROW_CODES)
    for names, s in ((T3_M, (p, m)), (T3_M1, (p, m + 1)), (T3_1, (p,)), (T3_NN, (p, n, n))):
        codes.update(names)
        shp.update({k: s for k in names})
    c = {}
    for name, code in codes.items():
        s = (nb,) + shp.get(name, (p, n, n))
        c[name] = h.debug_array(code, 0, int(np.prod(s))).reshape(s)
    if dm['rows']:
        c.update({'p' + k: v for k, v in h.debug_multipliers(nb, nr).items()})      # pphi, pz, pdphi, pdz: the multipliers of G / C
    c['iprob'] = h.debug_iprob(0, nb * IS).reshape(nb, IS)
    return c


def _call(h, case, prob, dm, rows=True):
    if not dm['rows'] or not rows:
        return h.convexify_step3_batch(prob['A'], prob['B'], prob['H'], prob['rho'])
    return h.convexify_step3_con_batch(prob['A'], prob['B'], prob['H'], prob['J'][:, :, :dm['nr']], prob['ncnt'], prob['rho'])


def run_case(prm, rows_generic=False, room=None):
    """the device calls of one case: -> dict(case, kind, K, dm, generic, solved, orient, s0, s1, s2, s3); rows_generic: TMPC_DEBUG_FLAG_GENERIC_ROWS;
    room: (ng, nc) the handle is made with when the plain Step 3 call runs on a handle with room for rows"""
    key = (prm, rows_generic, room)
    if key in _RUNS:
        return _RUNS[key]
    from tunempc_amd._lib import HipConvexifier, cr_schedule
    case, K, generic = prm
    dm = dims(case, room)
    prob = make_problem(case)
    c = dict(case=case, kind=K, dm=dm, generic=generic, solved=solved_members(case), orient=cr_schedule(dm['p'])['orient'])
    mk = lambda flags: HipConvexifier(dm['p'], dm['nx'], dm['mb'], chunk=dm['nb'], lanes=1, flags=flags, ng=dm['room'][0], nc=dm['room'][1], step3=True)
    if not isinstance(K, int):
        # scouting run: the whole solve on the launch sequence (what the stop flag forces), then column 1 of the trace: phase + 0.25 * chord
        h = mk(0)
        h.set_tuning(graph=0, persistent=0)
        _call(h, case, prob, dm)
        col = h.debug_array(CODES['trace'], 0, dm['nb'] * TRACE_LEN * TRACE_W).reshape(dm['nb'], TRACE_LEN, TRACE_W)[c['solved'][0], :, 1]
        h.close()
        hit = np.nonzero(col == (1.0 if K == 'center' else 1.25))[0]
        assert len(hit) > 0, f'the scouting run never reached a {K} iteration'
        K = int(hit[0]) + 1
    c['K'] = K
    h = mk(FLAG_STOP_ASSEMBLED | (FLAG_GENERIC_STAGE if generic else 0) | (FLAG_GENERIC_ROWS if rows_generic else 0))
    assert h.chunk == dm['nb']
    if room is not None and not dm['rows']:
        # a call WITH rows first (it stops at the assembled system of iteration 1): the multipliers' share of Q_RPHI2 / Q_NCONE, their rows of D, O, W3 and U stand
        # in the workspace when the calls without rows begin
        rng = np.random.default_rng(99)
        J = rng.standard_normal((dm['nb'], dm['p'], room[0] + room[1], dm['n']))
        h.convexify_step3_con_batch(prob['A'], prob['B'], prob['H'], J, np.full((dm['nb'], dm['p']), room[1], np.int32), prob['rho'])
        assert h.debug_array(CODES['part'], 0, NPART)[Q_NCONE] > dm['m'] + 1
    for name, point in STOPS:
        h.debug_set_stop_point(K, point)
        _call(h, case, prob, dm)
        c[name] = _snapshot(h, dm)
    h.close()
    _RUNS[key] = c
    return c


@pytest.fixture(scope='module', params=PARAMS, ids=_id)
def case(request):
    return run_case(request.param)


def members(c):
    """(b, phase, chord) of the members that iterate at the stop"""
    ip = c['s2']['iprob']
    return [(b, int(ip[b, I_PHASE]), int(ip[b, I_CHORD])) for b in c['solved'] if ip[b, I_PHASE] != PH_DONE]


def wr_of(c, snap, b):
    pr = snap['prob'][b]
    return c['case'][7] * pr[P_SBETA] / pr[P_S]


def stages(c, snap, b):
    """per stage: the Step 3 state and, with rows, the multiplier state (as tests/test_gpu_phi_kernels.py reads it) from the device arrays of one snapshot"""
    dm = c['dm']
    n, nx = dm['n'], dm['nx']
    out = []
    for k in range(dm['p']):
        s = dict(k=k, kn=(k + 1) % dm['p'], rows=0, arrows=[], nz=0)
        for name in list(T3_M) + list(T3_M1) + list(T3_1) + list(T3_NN):
            s[name] = snap[name][b, k]
        s['X'] = np.stack([snap['X1'][b, k], snap['X2'][b, k]]); s['Si'] = np.stack([snap['S1i'][b, k], snap['S2i'][b, k]])
        if dm['rows']:
            mr, arr = stage_layout(c['case'], k)
            s.update(rows=mr, arrows=[(e, a0, am) for e, (a0, am) in enumerate(arr)], nz=mr + len(arr))
            s['G'] = snap['G'][b, k, :mr]
            for name in ('phi', 'z', 'dphi', 'dz'):
                s['p' + name] = snap['p' + name][b, k, :mr]
            pv = snap['pvec'][b, k, :, :mr]
            s['w'], s['u'] = pv[..., :n], pv[..., n:2 * n]
            q = snap['psm'][b, k]; g = dm['nzs']
            s['pr'] = q[g * g + 4 * g:g * g + 4 * g + s['nz']]
            for e, a0, am in s['arrows']:
                s['aX', e] = snap['aX'][b, k, e, :am + 1, :am + 1]
                s['at', e], s['adt', e] = snap['at'][b, k, e], snap['adt'][b, k, e]
        out.append(s)
    return out


def _chk(got, ref, what):
    _inside(got, ref.v, ref.b, max(ref.m, 1), what)


ITERATE = ('X1', 'X2', 'S1', 'S2', 'P', 'V', 'Hb', 'S1i', 'S2i', 'th', 'z', 'x', 't', 'v', 'beta', 'lam')


# ------------------------------------------------------------------------------------------------------------------------------ 1. state at the stop, k_t3_init
def test_state_at_the_stop_points(case):
    """the phase the case is about, no lift and no frozen pivot; every member of solved_members iterates; row K of the trace absent before s3 and present at s3; what
    iteration K does not write between two points is bit-identical across the calls; K = 1: theta, z, t, x are the starting point of k_t3_init (x through
    1 / det: its bound carries kappa); K >= 2: theta has left it by more than 1e-2 relative; t > |w c o theta| and det x > 0 at s0 and after the step"""
    K, kind, dm = case['K'], case['kind'], case['dm']
    b0 = case['solved'][0]
    assert [m_[0] for m_ in members(case)] == case['solved']
    for b, phase, chord in members(case):
        for s in ('s0', 's1', 's2'):
            ip = case[s]['iprob'][b]
            assert ip[I_PHASE] == phase and ip[I_CHORD] == chord and ip[I_REG] == 0 and ip[I_NSHIFT] == ip[I_SHIFT0], (s, ip)
            assert not case[s]['trace'][b][K - 1:].any(), s
        row = case['s3']['trace'][b][K - 1]
        assert row[0] == K and row[1] == phase + 0.25 * chord and row[9] == 0.0, row
        if b == b0:
            assert (phase, chord) == dict(center=(1, 0), chord=(1, 1)).get(kind, (PH_MAIN, 0)), (phase, chord)
        g = [{k: v[b] for k, v in case[s].items()} for s in ('s0', 's1', 's2', 's3')]
        for i in (1, 2):
            for name in ITERATE:
                assert np.array_equal(g[0][name], g[i][name]), (name, f's0 vs s{i}')
        if phase == PH_MAIN:
            for name in ('cth', 'cq'):
                assert np.array_equal(g[1][name], g[2][name]), (name, 'the Mehrotra terms are written in pass 1 only')
        for name in ('dth', 'dz', 'dx', 'dt', 'g', 'dP', 'eigmin'):
            assert np.array_equal(g[2][name], g[3][name]), (name, 's2 vs s3')
        wr = wr_of(case, case['s0'], b)
        ref = t3.start(dm['p'], dm['n'], wr)
        for snap in ('s0', 's3'):
            for s in stages(case, case[snap], b):
                sl = t3.slack(s['t'], s['th'], wr, dm['n']).v
                assert t3.soc_inside(sl, 0 * sl, 0) and t3.soc_inside(s['x'], 0 * s['x'], 0) and (s['th'] > 0).all() and (s['z'] > 0).all(), (snap, s['k'])
        for s in stages(case, case['s0'], b):
            if K == 1:
                what = f'problem {b} stage {s["k"]} start'
                one = np.ones(dm['m'])
                _chk(s['th'], ref['th'] * one, what + ' theta'); _chk(s['z'], ref['z'] * one, what + ' z')
                _chk(s['t'], ref['t'], what + ' t'); _chk(s['x'], ref['x'], what + ' x')
                assert (ref['th'].v < 1) == (float(ref['x0'].v) * dm['n'] / wr < 1)
            else:
                assert np.linalg.norm(s['th'] - float(ref['th'].v)) > 1e-2 * np.linalg.norm(s['th']), ('theta still at its starting value', s['k'])
    for b in range(dm['nb']):
        if b not in case['solved']:
            assert case['s3']['iprob'][b, I_PHASE] == PH_DONE


# ------------------------------------------------------------------------------------------------------------------------------ 2. k_t3_pre
def _phi_part(case, snap, b, s):
    """the multipliers' share of Q_RPHI2, Q_XS, Q_NCONE as tests/test_gpu_phi_kernels.py holds it: -> (r2, r2 bound, xs, xs bound, cones, m)"""
    dm = case['dm']
    n, mr, nz = dm['n'], s['rows'], s['nz']
    if not dm['rows']:
        return LD(0), LD(0), LD(0), LD(0), 0, 0
    wr = wr_of(case, snap, b)
    GXG, GSG, GXb, GSb = ph.gram_products(s['G'], s['w'], s['u'])
    res, _ = ph.rows_residual(GXG, s['pz'])
    resb = ph.rows_residual(GXb, s['pz'])[1]
    res = np.concatenate([res, np.zeros(nz - mr, LD)]); resb = np.concatenate([resb, np.zeros(nz - mr, LD)])
    xs_arrows = []
    for e, a0, am in s['arrows']:
        X = s['aX', e]
        xs_arrows.append((X, np.asarray(ph.arrow(s['at', e], s['pphi'][a0:a0 + am], wr), float)))
        rq, rt, rqb, rtb = ph.arrow_residual(X, wr)
        res[a0:a0 + am] += rq; resb[a0:a0 + am] += rqb; res[mr + e] = rt; resb[mr + e] = rtb
    v, vb = ph.complementarity(s['pphi'], s['pz'], xs_arrows)
    return (np.sum(res * res), np.sum(resb * resb), v, vb, mr + sum(am + 1 for _, _, am in s['arrows']),
            2 * n + 9 + max(nz, 1) + mr + sum((am + 1) ** 2 for _, _, am in s['arrows']))


def test_t3_pre(case):
    """beta and v from the device t, theta, x (through 1 / sqrt(det s), 1 / sqrt(det x): the bound carries kappa(s) + kappa(x)); lambda = W x from the device beta, v,
    x; v'Jv = 1 inside the same conditioning; the partial sums Q_XS (LMIs + multipliers + theta'z + x's), Q_RPHI2 (accumulated behind the multipliers' share when
    the call has rows, set otherwise) and Q_NCONE"""
    dm = case['dm']
    n, m = dm['n'], dm['m']
    for b, phase, chord in members(case):
        snap = case['s0']
        wr = wr_of(case, snap, b)
        for s in stages(case, snap, b):
            what = f'problem {b} stage {s["k"]}'
            sl = t3.slack(s['t'], s['th'], wr, n)
            beta, v = t3.scaling(sl, s['x'])
            _chk(s['beta'], beta, what + ' beta'); _chk(s['v'], v, what + ' v')
            # v'Jv = 1 for the device v: each v_i within 4 gamma_m * bound_i of a vector whose det is 1, so |det v - 1| <= 2 sum |v_i| 4 gamma_m bound_i + its own rounding
            dv = t3.det(s['v'])
            assert abs(dv.v - 1) <= 2 * np.sum(np.abs(s['v']) * 4 * sr.gamma(v.m) * v.b) + 4 * sr.gamma(dv.m) * dv.b, (what, "v'Jv", float(dv.v))
            _chk(s['lam'], t3.scaled_point(s['beta'], s['v'], s['x']), what + ' lambda')
            part = snap['part'][b, s['k']]
            xs3, r23, nc3 = t3.pre_sums(s['t'], s['th'], s['z'], s['x'], s['X'][0], s['X'][1], wr, n)
            pr2, pr2b, pxs, pxsb, pnc, pm = _phi_part(case, snap, b, s)
            assert part[Q_NCONE] == nc3 + pnc, (what, part[Q_NCONE])
            _inside(np.array([part[Q_RPHI2]]), np.array([r23.v + pr2]), np.array([r23.b + pr2b]), r23.m + pm + 1, what + ' Q_RPHI2')
            xs = [np.sum(np.asarray(snap[f'X{r}'][b, s['k']], LD) * np.asarray(snap[f'S{r}'][b, s['k']], LD)) for r in (1, 2)]
            xsb = [np.sum(np.abs(snap[f'X{r}'][b, s['k']] * snap[f'S{r}'][b, s['k']])) for r in (1, 2)]
            _inside(np.array([part[Q_XS]]), np.array([xs[0] + xs[1] + pxs + xs3.v]), np.array([xsb[0] + xsb[1] + pxsb + xs3.b]), 2 * n * n + pm + xs3.m + 3, what + ' Q_XS')


# ------------------------------------------------------------------------------------------------------------------------------ 3. k_t3_schur, k_t3_cross
def _slot(case, O, k, rows, cols):
    return O[k][rows, cols] if case['orient'][k] == 0 else O[k][cols, rows].T


def test_t3_schur(case):
    """rows oT .. oT + m of block k+1: b in the first d columns of D (a + b at p = 1), a in the same rows of the coupling slot of stage k in the orientation of the
    schedule, the theta-theta block with the W^-2 and z / theta terms, the row of t, Ddiag = the diagonal written; with rows the block between theta and the
    multipliers (k_t3_cross, from the device pvec); the structure: columns d .. oT-1 of the row of t and the columns of absent rows are zero, the upper part of the
    diagonal block is not the mirror image of the lower (what a kernel that dropped its `j > oT + i` skip would write; the region holds what an earlier
    factorisation or the allocation left, so no value can be asserted), the padding behind row oT + m is the identity k_schur wrote, the slot outside the a rows is untouched"""
    dm = case['dm']
    p, nx, d, dp, m, oT, n = dm['p'], dm['nx'], dm['d'], dm['dp'], dm['m'], dm['oT'], dm['n']
    for b, phase, chord in members(case):
        if chord:
            continue                                               # a chord step assembles nothing
        snap = case['s0']
        D, O, Dd = snap['D'][b], snap['O'][b], snap['Ddiag'][b]
        wr = wr_of(case, snap, b)
        for s in stages(case, snap, b):
            k, kn = s['k'], s['kn']
            what = f'problem {b} stage {k}'
            R = t3.schur_rows(s['X'], s['Si'], snap['V'][b, k], s['beta'], s['v'], s['th'], s['z'], wr, nx)
            rows = slice(oT, oT + m)
            if p == 1:
                _chk(D[kn][rows, :d], R['a'] + R['b'], what + ' a + b in D')
            else:
                _chk(D[kn][rows, :d], R['b'], what + ' b in D of block k+1')
                _chk(_slot(case, O, k, rows, slice(0, d)), R['a'], what + ' a in the coupling slot')
            H = D[kn][rows, rows]
            low = np.tril(np.ones((m, m), bool))
            _inside(np.where(low, H, 0.0), np.where(low, R['H'].v, 0), np.where(low, R['H'].b, 0), R['H'].m, what + ' theta-theta block')
            # the upper part of the diagonal block is not k_t3_schur's to write (k_schur fills the lower part of the padding, the factorisation uses the rest as
            # it likes): it holds what an earlier factorisation or the allocation left; a kernel that wrote it would leave the mirror image of the lower part there
            up = np.triu(H, 1)
            if m > 1:
                assert not np.allclose(up, np.tril(H, -1).T, rtol=1e-6, atol=0, equal_nan=True), what + ': upper part of the diagonal block is the mirror image of the lower'
            _chk(D[kn][oT + m, oT:oT + m + 1], R['trow'], what + ' row of t')
            assert not D[kn][oT + m, :oT].any(), what + ': the row of t reaches P or the multipliers'
            assert np.array_equal(Dd[kn][oT:oT + m + 1], np.diagonal(D[kn])[oT:oT + m + 1]), what + ': Ddiag'
            assert np.array_equal(np.tril(D[kn])[oT + m + 1:, :], np.eye(dp)[oT + m + 1:, :]) and np.array_equal(Dd[kn][oT + m + 1:], np.ones(dp - oT - m - 1)), what + ': padding'
            if dm['rows']:
                _chk(D[kn][rows, d:d + s['rows']], t3.cross(s['w'], s['u'], n), what + ' theta x multipliers')
                assert not D[kn][rows, d + s['rows']:oT].any(), what + ': columns of absent rows and of the epigraph variables'
            Ok = O[k] if case['orient'][k] == 0 else O[k].T
            if p > 1:
                assert not Ok[oT + m:, :].any() and not Ok[oT:, d:].any(), what + ': padding of the coupling slot'
            else:
                assert not Ok[d:, :].any() and not Ok[:, d:].any(), what + ': the coupling slot at p = 1'


# ------------------------------------------------------------------------------------------------------------------------------ 4. k_t3_rhs, k_t3_gather
def test_rhs_and_gather(case):
    """g of k_t3_rhs in its three regimes -- pass 1 (s0 and s1: sig = 0, no Mehrotra term), pass 2 of the main phase (s2: sigma mu and cq of pass 1), centering (s2:
    mu_t WITHOUT cq, which still holds the term of the last main-phase iteration) -- through 1 / det s; the rows k_t3_gather writes at s0: the tails of W3
    (r | c_tau | c_alpha; c_tau, c_alpha bit-exact from the device Psi, Phi) and of U in block k+1, zeros behind them"""
    dm = case['dm']
    n, m, oT = dm['n'], dm['m'], dm['oT']
    for b, phase, chord in members(case):
        wr = wr_of(case, case['s0'], b)
        if phase == PH_MAIN:
            snap = case['s0']
            for s in stages(case, snap, b):
                what = f'problem {b} stage {s["k"]}'
                _chk(s['g'], t3.rhs_g(s['t'], s['th'], s['x'], None, 0.0, wr, n), what + ' g of pass 1')
                r, ct, ca = t3.gather_rows(snap['T1'][b, s['k']], snap['T2'][b, s['k']], s['th'], None, s['g'], s['x'], s['t3psi'], s['t3phi'], 0.0, wr, n)
                W3, U = snap['W3'][b, s['kn']], snap['U'][b, s['kn']]
                _chk(W3[oT:oT + m + 1, 0], r, what + ' right-hand side of pass 1')
                assert np.array_equal(W3[oT:oT + m, 1], ct) and np.array_equal(W3[oT:oT + m, 2], ca), what + ': c_tau, c_alpha in W3'
                assert np.array_equal(U[oT:oT + m], np.stack([ct, ca], axis=1)), what + ': U tail'
                assert not W3[oT + m, 1:].any() and not U[oT + m].any(), what + ': the row of t has no border entries'
                assert not W3[oT + m + 1:].any() and not U[oT + m + 1:].any(), what + ': padding of W3 / U'
        snap = case['s2']
        sig = snap['prob'][b][P_SIGMU]
        assert sig > 0.0
        for s in stages(case, snap, b):
            if phase != PH_MAIN:
                assert s['cq'].any()
            _chk(s['g'], t3.rhs_g(s['t'], s['th'], s['x'], s['cq'] if phase == PH_MAIN else None, sig, wr, n), f'problem {b} stage {s["k"]} g of pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 5. k_t3_dir
def _directions(case, snap, b, pass1, phase, what):
    dm = case['dm']
    n, m, oT = dm['n'], dm['m'], dm['oT']
    pr = snap['prob'][b]
    wr = wr_of(case, snap, b)
    sig = 0.0 if pass1 else pr[P_SIGMU]
    use_corr = (not pass1) and phase == PH_MAIN
    for s in stages(case, snap, b):
        w_ = what + f' stage {s["k"]}'
        dy = t3.local_direction(snap['Z'][b, s['kn'], oT:oT + m + 1], snap['TU'][b, s['kn'], oT:oT + m + 1], pr[P_DTAU], pr[P_DALPHA])
        _chk(s['dth'], dy[:m], w_ + ' dtheta'); _chk(s['dt'], dy[m], w_ + ' dt')
        # the cth the kernel reads in pass 2 is the one pass 1 wrote: at s2 it still stands (bit-identical to s1, test_state_at_the_stop_points)
        dz = t3.dual_direction(s['th'], s['z'], s['dth'], sig, s['cth'] if use_corr else None)
        _chk(s['dz'], dz, w_ + ' dz')
        ds = t3.cone_ds(s['dt'], s['dth'], wr, n)
        _chk(s['dx'], t3.cone_dx(s['g'], s['beta'], s['v'], ds), w_ + ' dx')
        # ... and dx = g - W^-2 ds with the dense W^-2 of the general formula (not the rank-two form the kernel and cone_dx share)
        W2 = t3.w2inv(s['beta'], s['v'])
        _chk(s['dx'], t3.VB(s['g']) - W2 @ ds, w_ + ' dx = g - W^-2 ds')
        # linearised complementarity of the linear cone: z dth + th dz = sig - th z - th cth
        lhs = t3.VB(s['z']) * t3.VB(s['dth']) + t3.VB(s['th']) * t3.VB(s['dz'])
        rhs = sig - t3.VB(s['th']) * t3.VB(s['z']) - (t3.VB(s['th']) * t3.VB(s['cth']) if use_corr else 0.0)
        res = lhs - rhs
        assert (np.abs(res.v) <= 4 * sr.gamma(res.m + 7) * res.b).all(), w_ + ' z dth + th dz = sig - th z - corr'
        if pass1:
            _chk(s['cth'], t3.mehrotra_theta(s['dz'], s['dth'], s['th']), w_ + ' cth')
            _chk(s['cq'], t3.cone_mehrotra(s['beta'], s['v'], s['lam'], s['dx'], ds), w_ + ' cq')


def test_directions(case):
    """dtheta, dt (the tail of the block solution), dz, dx (rank-two form and dense W^-2), in pass 1 the Mehrotra terms cth and cq = W^-1 (lambda \\ ((W dx) o (W^-1 ds)))
    (through 1 / det lambda: the bound carries kappa(lambda)) -- both passes, from the device Z, TU, dtau, dalpha, theta, z, g, beta, v, lambda"""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _directions(case, case['s1'], b, True, phase, f'problem {b} pass 1')
        _directions(case, case['s2'], b, False, phase, f'problem {b} pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 6. local Newton rows
def _dense_system(case, b, phase):
    """the system assembled at s0 as one dense symmetric matrix [p dp + 2] (tests/test_gpu_phi_kernels.py: _dense_system)"""
    dm = case['dm']
    p, dp = dm['p'], dm['dp']
    s0 = case['s0']
    N = p * dp
    Kd = np.zeros((N + 2, N + 2))
    for k in range(p):
        kn = (k + 1) % p
        Dk = np.tril(s0['D'][b, k]); Dk = Dk + np.tril(Dk, -1).T
        Kd[k * dp:(k + 1) * dp, k * dp:(k + 1) * dp] += Dk
        C = s0['O'][b, k] if case['orient'][k] == 0 else s0['O'][b, k].T          # T[block k+1, block k]
        Kd[kn * dp:(kn + 1) * dp, k * dp:(k + 1) * dp] += C
        Kd[k * dp:(k + 1) * dp, kn * dp:(kn + 1) * dp] += C.T
    U = (s0 if phase == PH_MAIN else case['s2'])['U'][b].reshape(N, 2)
    Kd[:N, N:] = U; Kd[N:, :N] = U.T
    pr = case['s1' if phase == PH_MAIN else 's2']['prob'][b]
    Kd[N:, N:] = [[pr[P_BTT], pr[P_BTA]], [pr[P_BTA], pr[P_BAA]]]
    return Kd


def _device_solution(case, snap, b):
    dm = case['dm']
    p, d, dp, nx, oT, m = dm['p'], dm['d'], dm['dp'], dm['nx'], dm['oT'], dm['m']
    ia, ib = sr.tri_idx(nx)
    x = np.zeros(p * dp + 2)
    for k in range(p):
        x[k * dp:k * dp + d] = snap['dP'][b, k][ia, ib]
    for s in stages(case, snap, b):
        o = s['kn'] * dp
        if dm['rows']:
            x[o + d:o + d + s['rows']] = s['pdphi']
            for e, _, _ in s['arrows']:
                x[o + d + s['rows'] + e] = s['adt', e]
        x[o + oT:o + oT + m] = s['dth']; x[o + oT + m] = s['dt']
    x[-2:] = snap['prob'][b][[P_DTAU, P_DALPHA]]
    return x


def _t3_rows_residual(case, b, Kd, rhs, x):
    """largest residual of the rows of (theta_k, t_k) of Kd x = rhs relative to the largest term of those rows"""
    dm = case['dm']
    worst = 0.0
    for k in range(dm['p']):
        rows = ((k + 1) % dm['p']) * dm['dp'] + dm['oT'] + np.arange(dm['m'] + 1)
        res = Kd[rows] @ x - rhs[rows]
        scale = np.abs(Kd[rows]) @ np.abs(x) + np.abs(rhs[rows])
        worst = max(worst, float(np.max(np.abs(res) / scale)))
    return worst


def t3_newton_residuals(case, b, phase):
    """[(pass, device, reference)]: the residual of the rows of (theta, t) of the system assembled at s0 with the device direction and with the direction of a dense
    fp64 LAPACK solve of that system (floored at 2^-53); the pass-2 right-hand side is rebuilt from the device arrays of s2 (the solve overwrote it)"""
    dm = case['dm']
    p, dp, nx, d, oT, m, n = dm['p'], dm['dp'], dm['nx'], dm['d'], dm['oT'], dm['m'], dm['n']
    N = p * dp
    Kd = _dense_system(case, b, phase)
    out = []
    for pas, snap in ((1, case['s1']), (2, case['s2'])):
        if pas == 1 and phase != PH_MAIN:
            continue
        pr = snap['prob'][b]
        rhs = np.zeros(N + 2)
        if pas == 1:
            rhs[:N] = case['s0']['W3'][b][:, :, 0].ravel()
            sig, corr0, part = 0.0, 0.0, case['s0']['part'][b]
        else:
            g = {k: snap[k][b] for k in ('T1', 'T2', 'X1', 'X2', 'S1i', 'S2i', 'Hb', 'V')}
            cols = np.asarray(sr.rhs_columns(g['T1'], g['T2'], g['X1'], g['X2'], g['S1i'], g['S2i'], g['Hb'], g['V'], nx)[0][:, :, 0], float)
            r3 = rhs[:N].reshape(p, dp)
            r3[:, :d] = cols
            sig, corr0, part = pr[P_SIGMU], pr[P_CORR0], snap['part'][b]
            wr = wr_of(case, snap, b)
            for s in stages(case, snap, b):
                if dm['rows']:
                    r3[s['kn'], d:d + s['nz']] = s['pr']
                r = t3.gather_rows(g['T1'][s['k']], g['T2'][s['k']], s['th'], s['cth'] if phase == PH_MAIN else None, s['g'], s['x'], s['t3psi'], s['t3phi'], sig, wr, n)[0]
                r3[s['kn'], oT:oT + m + 1] = np.asarray(r.v, float)
        t0 = sig / pr[P_S0] - pr[P_X0] * pr[P_RD0] / pr[P_S0] - corr0
        rhs[N:] = [part[:, Q_TRT2].sum() - 1.0, part[:, Q_HBG].sum() + t0]
        ref = np.linalg.solve(Kd, rhs)
        out.append((pas, _t3_rows_residual(case, b, Kd, rhs, _device_solution(case, snap, b)), max(_t3_rows_residual(case, b, Kd, rhs, ref), 2.0 ** -53)))
    return out


def test_local_newton_rows(case):
    """The directions satisfy the rows of (theta_k, t_k) of the Newton equations of the system the kernels assembled: ties k_t3_schur, k_t3_cross, k_t3_gather, the
    block solve, the border solve and k_t3_dir's tail read together.  The error of a solve has no rounding bound, so the device residual is held against that of a
    dense fp64 LAPACK solve of the same assembled system by NEWTON_RESIDUAL_FACTOR['fp64'] (Step 3 never iterates in float32: run_chunk turns the switch off);
    a chord step's system is not in the workspace"""
    for b, phase, chord in members(case):
        if chord:
            continue
        for pas, dev, ref in t3_newton_residuals(case, b, phase):
            print(f't3-newton-residual {_id((case["case"], case["kind"], case["generic"]))} problem {b} pass {pas}: device {dev:.3e} reference {ref:.3e} ratio {dev / ref:.3g}')
            assert ref <= 1e-6, (b, pas, ref)
            assert dev <= NEWTON_RESIDUAL_FACTOR['fp64'] * ref, (b, pas, dev, ref, dev / ref)


# ------------------------------------------------------------------------------------------------------------------------------ 7. k_t3_steps
def _root_ok(u, du, eig):
    """eig = -1 / th is the cone's step length: th a root of the boundary inside the tolerance of the pair, 0.999 th strictly inside, no smaller positive root"""
    if eig >= 0.0:
        return t3.soc_step_bisect(u, du) == np.inf
    th = -1.0 / eig
    ref = t3.soc_step_bisect(u, du)
    return bool(np.isfinite(ref) and th <= ref * (1 + 1e-6) and t3.soc_inside(u, du, 0.999 * th) and t3.soc_root_residual(u, du, th) <= _root_tol(u, du))


def _restatement_floor(m1):
    """largest root residual the fp64 restatement leaves on the edge pairs of section c of length m1"""
    if m1 not in _FLOOR:
        res = [t3.soc_root_residual(u, du, -1.0 / e) for _, u, du in _edge_pairs(m1) for e in [t3.soc_step_eig64(u, du)] if e < 0]
        _FLOOR[m1] = max(res)
    return _FLOOR[m1]


def _root_tol(u, du):
    """SOC_ROOT_FACTOR * max((i) the residual of the fp64 restatement's root on the same pair, (ii) its worst residual on the edge pairs of the same length,
    (iii) the residual of the exact root (bisection in longdouble) moved by 2 eps relative)"""
    e64 = t3.soc_step_eig64(u, du)
    ref = LD(t3.soc_step_bisect(u, du))
    a, bq, _ = t3.soc_poly(u, du)
    w = np.asarray(u, LD) + ref * np.asarray(du, LD)
    moved = float(abs(2 * (bq + a * ref) * ref) * 2 * EPS / (w @ w))
    return SOC_ROOT_FACTOR * max(_restatement_floor(len(u)), t3.soc_root_residual(u, du, -1.0 / e64) if e64 < 0 else 0.0, moved)


def _steps(case, snap, b, phase, pass2, what):
    dm = case['dm']
    n, m = dm['n'], dm['m']
    g = {k: v[b] for k, v in snap.items()}
    wr = wr_of(case, snap, b)
    X, S, dX, dS = ([np.asarray(g[a + r], LD) for r in '12'] for a in ('X', 'S', 'dX', 'dS'))
    f = lambda A, B, fn: sum(np.sum(fn(A[r] * B[r]), axis=(1, 2)) for r in (0, 1))
    v = np.stack([f(dX, S, lambda t: t), f(X, dS, lambda t: t), f(dX, dS, lambda t: t)], axis=1)
    vb = np.stack([f(dX, S, np.abs), f(X, dS, np.abs), f(dX, dS, np.abs)], axis=1)
    ev = np.linalg.eigvalsh(g['Wm'])
    th = eig_thresholds(phase)
    for s in stages(case, snap, b):
        k = s['k']
        sl, ds = t3.slack(s['t'], s['th'], wr, n), t3.cone_ds(s['dt'], s['dth'], wr, n)
        sm = t3.sums(s['th'], s['z'], s['dth'], s['dz'], sl, ds, s['x'], s['dx'])
        lv, lb, asum, lin = np.zeros(3, LD), np.zeros(3, LD), np.zeros(5), (0.0, 0.0)
        if dm['rows']:
            lv, lb = ph.linear_cone_sums(s['pphi'], s['pz'], s['pdphi'], s['pdz'])
            asum = g['asum'][k]
            lin = ph.linear_cone_steps(s['pphi'], s['pz'], s['pdphi'], s['pdz']) if s['rows'] else (0.0, 0.0)
        for j, q in enumerate((Q_DXS, Q_XDS, Q_DXDS)):
            _inside(np.array([g['part'][k, q]]), np.array([v[k, j] + lv[j] + LD(asum[j]) + sm[j].v]), np.array([vb[k, j] + lb[j] + abs(LD(asum[j])) + sm[j].b]),
                    2 * n * n + s['rows'] + sm[j].m + 4, what + f' stage {k} partial sum {j}')
        ls, lx = t3.linear_steps(s['th'], s['z'], s['dth'], s['dz'])
        cone = ((np.asarray(sl.v, float), np.asarray(ds.v, float)), (s['x'], s['dx']))
        for slot, fold in ((0, min(ls, lin[0], asum[3])), (1, min(lx, lin[1], asum[4]))):
            got, ref, scale = g['eigmin'][k, slot], ev[k, slot, 0], np.abs(ev[k, slot]).max()
            u, du = cone[slot]
            cref = t3.soc_step_bisect(u, du)
            cone_eig = 0.0 if cref == np.inf else -1.0 / cref
            assert got <= fold, (what, k, slot, got, fold)
            # the cone's own value is in the minimum: either something else is smaller still, or the value written is the cone's root
            assert got <= cone_eig * (1 - 1e-6) or _root_ok(u, du, got), (what, k, slot, 'the cone is not in the minimum', got, cone_eig)
            if got == fold:
                assert ref >= fold - 1e-12 * scale, (what, k, slot, got, ref)
            elif not _root_ok(u, du, got):
                # neither a linear-cone ratio nor the cone's root: the LMI's eigenvalue, or (pass 2 of k_eigmin) the bound -1 / theta of its pre-test
                assert abs(got - ref) <= 1e-12 * scale or (pass2 and any(got == -1.0 / t and ref > got for t in th)), (what, k, slot, got, ref)
            else:
                assert ref >= got - 1e-12 * scale or (pass2 and any(ref > -1.0 / t for t in th)), (what, k, slot, got, ref)


def test_steps_fold(case):
    """what k_t3_steps folds into the step-length minima and the mu_aff sums: eigmin[0] = min(LMI 1's dual answer, min dphi / phi and the arrows' minimum of the
    multipliers, min dtheta / theta, the cone's step for (s, ds)) and eigmin[1] likewise with dz / z and (x, dx) -- the linear-cone ratios bit-exact, the cone's
    value accepted as a root (SOC_ROOT_FACTOR) that bisection confirms as the first exit; Q_DXS, Q_XDS, Q_DXDS = the two LMIs + the multipliers + the Step 3 part"""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _steps(case, case['s1'], b, phase, False, f'problem {b} pass 1')
        _steps(case, case['s2'], b, phase, True, f'problem {b} pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 8. k_t3_update
def test_update(case):
    """theta and t move by ad, z and x by ap, exactly the step times the direction (m = 2); the cone constraints still hold (test_state_at_the_stop_points); a member
    that left at the pre-check keeps its state bit for bit"""
    dm = case['dm']
    for b, phase, chord in members(case):
        y = case['s3']
        ap, ad = y['prob'][b][P_AP], y['prob'][b][P_AD]
        assert ap > 0.0 and ad > 0.0
        for s2, s3 in zip(stages(case, case['s2'], b), stages(case, y, b)):
            what = f'problem {b} stage {s2["k"]}'
            for name, dname, a in (('th', 'dth', ad), ('t', 'dt', ad), ('z', 'dz', ap), ('x', 'dx', ap)):
                _chk(s3[name], t3.update(s2[name], s2[dname], a), what + ' updated ' + name)
                assert not np.array_equal(s3[name], s2[name])
    idle = [b for b in range(dm['nb']) if b not in case['solved']]
    for b in idle:
        for name in ('th', 'z', 'x', 't'):
            assert np.array_equal(case['s0'][name][b], case['s3'][name][b]), (b, name)
    if dm['nb'] == 3:
        assert idle == [1]


def test_cases_tell_ap_from_ad():
    """across the small main-phase cases some step has ap != ad: test_update would not tell the two apart otherwise"""
    assert any(run_case(prm)['s3']['prob'][b][P_AP] != run_case(prm)['s3']['prob'][b][P_AD] for prm in MAIN_CASES if prm[0] not in LARGE_CASES and not prm[2]
               for b, _, _ in members(run_case(prm)))


# ------------------------------------------------------------------------------------------------------------------------------ 9. soc_step_eig at its edges
def _edge_pairs(m1):
    from test_t3_reference_cpu import step_pairs
    return step_pairs(m1)


@pytest.mark.parametrize('m1', [2, 64, 65, 67, 529])
def test_soc_step_at_its_edges(m1):
    """soc_step_eig through tmpc_debug_soc_step: du inside the cone and on its boundary with bq > 0 (unbounded: 0), du on the boundary of -Q (a = 0 exactly), du in -Q,
    du0 < 0 outside both cones, u at relative distance 1e-8 from the boundary, du within 1e-6 .. 1e-15 of the boundary of -Q (a > 0 with few digits), random pairs.
    A returned th = -1 / eig is accepted if det(u + th du) is zero inside the tolerance of the pair (SOC_ROOT_FACTOR), 0.999 th is strictly inside and
    bisection finds no smaller positive root"""
    from tunempc_amd._lib import HipConvexifier
    pairs = _edge_pairs(m1)
    h = HipConvexifier(2, 2, 1, chunk=1, lanes=1)
    eig = h.debug_soc_step(np.stack([u for _, u, _ in pairs]), np.stack([du for _, _, du in pairs]))
    h.close()
    for (name, u, du), e in zip(pairs, eig):
        ref = t3.soc_step_bisect(u, du)
        res = t3.soc_root_residual(u, du, -1.0 / e) / EPS if e < 0 else 0.0
        print(f'soc-step m1 {m1} {name}: eig {e!r} bisection {ref!r} residual {res:.3g} eps tolerance {_root_tol(u, du) / EPS if ref != np.inf else 0:.3g} eps')
        if ref == np.inf:
            assert e == 0.0, name
            continue
        assert e < 0.0 and _root_ok(u, du, e), (name, e, ref, res)
        assert abs(-1.0 / e - ref) <= 1e-6 * ref, (name, 'not the first exit', -1.0 / e, ref)


# ------------------------------------------------------------------------------------------------------------------------------ 10. the forms
@pytest.mark.parametrize('prm', [q for q in MAIN_CASES if not q[2] and q[0] in SMALL_CASES], ids=_id)
def test_generic_rows_form_returns_the_same_bits(prm):
    """k_t3_schur<true> (X_r, S_r^-1 read where they lie, X_r V' and S_r^-1 V' in the stage scratch) at n <= 32 behind the tuned stage kernels
    (TMPC_DEBUG_FLAG_GENERIC_ROWS): the same arithmetic in the same order on bit-identical inputs -- D, O, Ddiag and everything that follows are the same bits"""
    tuned, rows = run_case(prm), run_case(prm, rows_generic=True)
    for b, phase, chord in members(tuned):
        for name in ('X1', 'X2', 'S1i', 'S2i', 'V', 'v', 'beta', 'th', 'z'):
            assert np.array_equal(tuned['s0'][name][b], rows['s0'][name][b]), (name, 'inputs of k_t3_schur')
        assert np.array_equal(np.tril(tuned['s0']['D'][b]), np.tril(rows['s0']['D'][b])), 'D'
        for name in ('O', 'Ddiag', 'W3', 'U'):
            assert np.array_equal(tuned['s0'][name][b], rows['s0'][name][b]), name
        for snap in ('s2', 's3'):
            for name in ('dth', 'dz', 'dx', 'dt', 'th', 'z', 'x', 't', 'dP', 'eigmin', 'P', 'X1', 'S1'):
                assert np.array_equal(tuned[snap][name][b], rows[snap][name][b]), (snap, name)


@pytest.mark.parametrize('K', (1, 2, 5))
def test_room_for_rows_without_rows_returns_the_same_bits(K):
    """a handle with room for rows (ng = 1, nc = 2) called without rows returns the bits of a handle without room: the same block size, Q_RPHI2 / Q_NCONE set, not
    accumulated on what a former call with rows left (run_case makes such a call on the handle with room first), nothing of that call's rows left in D, O, W3, U"""
    plain, room = run_case((P2, K, False)), run_case((P2, K, False), room=(1, 2))
    assert plain['dm']['dp'] == room['dm']['dp']
    written_at_s0 = ITERATE + ('D', 'O', 'Ddiag', 'W3', 'U', 'part', 'T1', 'T2', 'g', 't3psi', 't3phi', 'prob', 'trace')
    for snap in ('s0', 's2', 's3'):
        for name in list(CODES) + list(T3_M) + list(T3_M1) + list(T3_1) + list(T3_NN):
            if snap == 's0' and name not in written_at_s0:
                continue                                           # (the directions and what follows them: not written yet at the first stop of a handle)
            if name in ('D',):
                assert np.array_equal(np.tril(plain[snap][name]), np.tril(room[snap][name])), (snap, name)
            elif name == 'part':                                   # the sums written by this stop point (the others hold what the allocation held)
                cols = [Q_XS, Q_RPHI2, Q_NCONE, Q_TRT2, Q_HBG] + ([Q_DXS, Q_XDS, Q_DXDS] if snap != 's0' else [])
                assert np.array_equal(plain[snap][name][..., cols], room[snap][name][..., cols]), (snap, name)
            else:
                assert np.array_equal(plain[snap][name], room[snap][name], equal_nan=True), (snap, name)


# ------------------------------------------------------------------------------------------------------------------------------ 11. the read-back itself
def test_step3_codes_without_step3_state_are_refused():
    """codes 54 .. 69 of tmpc_debug_get_array: TMPC_E_ARG on a handle without room for T, and on a handle with room after a call that ran without Step 3 (nT = 0);
    after a Step 3 call on the same handle they read"""
    from tunempc_amd._lib import HipConvexifier
    prob = make_problem(P2)
    nb, p, nx, mb = P2[:4]
    h = HipConvexifier(p, nx, mb, chunk=nb, lanes=1)
    h.convexify_batch(prob['A'], prob['B'], prob['H'])
    for code in range(54, 70):
        with pytest.raises(RuntimeError):
            h.debug_array(code, 0, 1)
    h.close()
    h = HipConvexifier(p, nx, mb, chunk=nb, lanes=1, step3=True)
    for code in range(54, 70):
        with pytest.raises(RuntimeError):                          # no call yet
            h.debug_array(code, 0, 1)
    h.convexify_step3_batch(prob['A'], prob['B'], prob['H'], prob['rho'])
    assert all(np.isfinite(h.debug_array(code, 0, 1)).all() for code in range(54, 70))
    h.convexify_batch(prob['A'], prob['B'], prob['H'])
    for code in range(54, 70):
        with pytest.raises(RuntimeError):
            h.debug_array(code, 0, 1)
    with pytest.raises(RuntimeError):
        h.debug_array(70, 0, 1)
    h.close()
