"""Kernel-level check of the rows of the stage-local multipliers (tunempc_amd/csrc/tmpc_phi.h): k_phi_pre in its four <BIGN, BIGR> forms, k_aug_fill,
k_phi_rhs, k_aug_gather, k_phi_dir with kb_phi_dm, k_phi_steps and k_phi_update -- Step 1 with G and Step 2 -- at iterates the SOLVER reached.  A call runs
iterations 1 .. K-1 as always and stops inside iteration K at one of four points (TMPC_DEBUG_FLAG_STOP_ASSEMBLED + tmpc_debug_set_stop_point):
    s0  the assembled system and the pass-1 right-hand sides        s1  after pass 1 and k_ctrl_b        s2  pass 2 complete, before k_ctrl_c        s3  iteration K complete
one device call per point, all on one handle with chunk = batch and lanes = 1 (tmpc_debug_get_array reads lane 0).

Every layer is compared with tests/phi_reference.py (numpy, np.longdouble) evaluated on that layer's OWN device inputs: |device - reference| <= 4 gamma_m * bound
entrywise, m counted at each assert (tests/test_gpu_schur_assembly.py explains the form).  Exceptions, by the rules of the two sibling files: the inverses of the arrow
blocks are held by their residual against the condition number; step-length eigenvalues against eigvalsh at 1e-12 of the matrix's scale; the block solve has no
rounding bound, so the stage-local rows of the Newton equations are held against a dense fp64 LAPACK solve of the system assembled at s0 (NEWTON_RESIDUAL_FACTOR of
tests/test_gpu_step_kernels.py).  Cases: tests/phi_kernel_cases.py.

Not covered here: a chord step's local Newton rows (its system is not in the workspace: D holds the factor of an earlier iterate), the
double-double assembly (k_dd_aug_fill) and the persistent kernel.  Step 3 (tmpc_t3.h) with and without these rows: tests/test_gpu_t3_kernels.py."""
import numpy as np
import pytest

import phi_reference as ph
import schur_reference as sr
import step_reference as st
from phi_kernel_cases import (BIGR_CASE, BIGR_TWIN_NC, CENTER_CASES, LARGE_CASES, MAIN_CASES, make_problem, solved_members, stage_layout)
from step_kernel_cases import (I_CHORD, I_LOWP, I_NSHIFT, I_PHASE, I_REG, I_SHIFT0, IS, NPART, P_AD, P_AP, P_BAA, P_BTA, P_BTT, P_CORR0, P_DALPHA, P_DTAU, P_RD0, P_S0, P_SIGMU,
                               P_X0, PH_DONE, PH_MAIN, PS, Q_DXDS, Q_DXS, Q_HBG, Q_TRT2, Q_XDS, TRACE_LEN, TRACE_W, eig_thresholds)
from test_gpu_schur_assembly import _inside
from test_gpu_step_kernels import NEWTON_RESIDUAL_FACTOR

pytestmark = pytest.mark.gpu

LD = sr.LD
FLAG_STOP_ASSEMBLED, FLAG_GENERIC_STAGE, FLAG_GENERIC_ROWS = 8, 64, 128
STOPS = (('s0', 0), ('s1', 1), ('s2', 2), ('s3', 3))
P_S, P_SBETA, Q_XS, Q_RPHI2, Q_NCONE = 9, 10, 0, 24, 25           # csrc/tmpc_common.h
AEL = 32                                                          # row stride of the arrow arrays
CODES = dict(psm=0, pvec=1, Ddiag=2, D=3, part=4, O=5, W3=7, U=8, X1=9, X2=10, S1=11, S2=12, P=13, V=14, Hb=15, S1i=16, S2i=17, T1=20, T2=21, Z=25, prob=26, trace=27,
             dP=28, dX1=29, dX2=30, dS1=31, dS2=32, Wm=39, eigmin=40, TU=41, G=42, corrp=43, asum=52)
ARROW_CODES = dict(at=44, adt=45, aX=46, adX=47, acor=48, aSi=49, aLi=50, aLXi=51)
PRS = 53
# the factor by which the device's residual of the stage-local Newton rows may exceed that of a dense fp64 LAPACK solve of the same assembled system
# (test_local_newton_rows): 'fp64' is NEWTON_RESIDUAL_FACTOR of tests/test_gpu_step_kernels.py; 'float32' (a main-phase iteration whose Schur-complement updates
# and triangular solves ran in float32) needs its own: this residual is relative to the terms of its own rows, so a float32 solve leaves ~2^-24 where the
# reference leaves ~2^-53 -- a ratio of the two unit roundings, 5.4e8, whatever the conditioning.  Measured against the dense reference
# (profiles/phi_kernel_residuals.txt: largest 5.05e8), rounded up to the next power of ten like the factors of that file.
# 'center' (the first centering iteration, a new fp64 factorisation at an iterate near the boundary): 67.2 as the kernels stand, and 1146 with the two Gram factors
# of T_loc,loc multiplied in the other, equally valid order (mutation 2 of profiles/phi_kernel_mutations.txt: the same number up to rounding) -- the residual of
# this iterate swings with the last bits of the matrix, so the larger of the two is the measurement, rounded up likewise.
LOCAL_NEWTON_FACTOR = dict(fp64=NEWTON_RESIDUAL_FACTOR['fp64'], float32=1e9, center=1e4)
PARAMS = MAIN_CASES + CENTER_CASES
_RUNS = {}


def _id(prm):
    (nb, p, nx, mb, ng, nc, ncnt, rho), k, generic = prm
    return (f'nb{nb}-p{p}-nx{nx}-mb{mb}-ng{ng}-nc{nc}-' + ('eq' if ncnt is None else ('norm' if rho > 0 else 'free')) + '-' + (f'K{k}' if isinstance(k, int) else k)
            + ('-generic' if generic else ''))


def dims(case, nc_room=None):
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    nc = nc if nc_room is None else nc_room
    n = nx + mb; d = nx * (nx + 1) // 2
    nr = ng + nc
    nzs = nr + (2 if (ncnt is not None and rho > 0.0) else 0)     # run_chunk: the epigraph variables only with norm terms
    return dict(nb=nb, p=p, nx=nx, mb=mb, n=n, d=d, ng=ng, nc=nc, nr=nr, nzs=nzs, dp=(d + nzs + 15) // 16 * 16, arrows=nc > 0, prs=nr > 32)


def _snapshot(h, dm):
    nb, p, nx, n, dp, nr, nzs = (dm[k] for k in ('nb', 'p', 'nx', 'n', 'dp', 'nr', 'nzs'))
    shp = dict(psm=(p, nzs * nzs + 6 * nzs), pvec=(p, 2, nr, 2 * n + 2 * nx), Ddiag=(p, dp), D=(p, dp, dp), O=(p, dp, dp), part=(p, NPART), W3=(p, dp, 3), U=(p, dp, 2),
               TU=(p, dp, 2), Z=(p, dp), P=(p, nx, nx), dP=(p, nx, nx), V=(p, nx, n), prob=(PS,), trace=(TRACE_LEN, TRACE_W), Wm=(p, 4, n, n), eigmin=(p, 4),
               G=(p, nr, n), corrp=(p, nr), asum=(p, 5), at=(p, 2), adt=(p, 2))
    c = {}
    codes = dict(CODES)
    if dm['arrows']:
        codes.update(ARROW_CODES)
    if dm['prs']:
        codes['prs'] = PRS
        shp['prs'] = (p, 4, nr, nr)
    for name, code in codes.items():
        s = (nb,) + shp.get(name, (p, 2, AEL, AEL) if name in ARROW_CODES else (p, n, n))
        c[name] = h.debug_array(code, 0, int(np.prod(s))).reshape(s)
    c.update(h.debug_multipliers(nb, nr))
    c['iprob'] = h.debug_iprob(0, nb * IS).reshape(nb, IS)
    return c


def _call(h, case, prob, dm):
    J = prob['J'][:, :, :dm['nr']]
    if case[6] is None:
        return h.convexify_eq_batch(prob['A'], prob['B'], prob['H'], J)
    return h.convexify_step2_batch(prob['A'], prob['B'], prob['H'], J, prob['ncnt'], prob['rho'])


def run_case(prm, nc_room=None, rows_generic=False):
    """the device calls of one case: -> dict(case, kind, K, dm, generic, solved, orient, s0, s1, s2, s3); nc_room: another room for rows of C than the case's;
    rows_generic: TMPC_DEBUG_FLAG_GENERIC_ROWS"""
    key = (prm, nc_room) + ((True,) if rows_generic else ())
    if key in _RUNS:
        return _RUNS[key]
    from tunempc_amd._lib import HipConvexifier, cr_schedule
    case, K, generic = prm
    dm = dims(case, nc_room)
    prob = make_problem(case)
    c = dict(case=case, kind=K, dm=dm, generic=generic, solved=solved_members(case), absent=False, orient=cr_schedule(dm['p'])['orient'])
    mk = lambda flags: HipConvexifier(dm['p'], dm['nx'], dm['mb'], chunk=dm['nb'], lanes=1, flags=flags, ng=dm['ng'], nc=dm['nc'])
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
    for name, point in STOPS:
        h.debug_set_stop_point(K, point)
        _call(h, case, prob, dm)
        c[name] = _snapshot(h, dm)
    if not dm['prs']:
        with pytest.raises(RuntimeError):                          # an array the handle does not have: TMPC_E_ARG, as the header promises
            h.debug_array(PRS, 0, 1)
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
    """per stage: dict(k, kn, m rows present, arrows [(e, a0, am)], nz, G, phi, z, X, Si [2, n, n], ...) from the device arrays of one snapshot"""
    dm = c['dm']
    out = []
    for k in range(dm['p']):
        m, arr = stage_layout(c['case'], k)
        m = min(m, dm['nr'])
        s = dict(k=k, kn=(k + 1) % dm['p'], m=m, arrows=[(e, a0, am) for e, (a0, am) in enumerate(arr)], nz=m + len(arr))
        s['G'] = snap['G'][b, k, :m]
        for name in ('phi', 'z', 'dphi', 'dz', 'corrp'):
            s[name] = snap[name][b, k, :m]
        s['X'] = np.stack([snap['X1'][b, k], snap['X2'][b, k]]); s['Si'] = np.stack([snap['S1i'][b, k], snap['S2i'][b, k]])
        pv = snap['pvec'][b, k, :, :m]
        n, nx = dm['n'], dm['nx']
        s['w'], s['u'], s['Vw'], s['Vu'] = pv[..., :n], pv[..., n:2 * n], pv[..., 2 * n:2 * n + nx], pv[..., 2 * n + nx:]
        q = snap['psm'][b, k]; g = dm['nzs']
        s['K'] = q[:g * g].reshape(g, g)[:s['nz'], :s['nz']]
        s['ct'], s['ca'], s['r'] = (q[g * g + j * g:g * g + j * g + s['nz']] for j in (0, 1, 4))
        for e, a0, am in s['arrows']:
            ne = am + 1
            for name in ('aX', 'adX', 'acor', 'aSi', 'aLi', 'aLXi'):
                s[name, e] = snap[name][b, k, e, :ne, :ne]
            s['at', e], s['adt', e] = snap['at'][b, k, e], snap['adt'][b, k, e]
        out.append(s)
    return out


def _bit_equal(a, z, names, what):
    for k in names:
        if k in a:
            assert np.array_equal(a[k], z[k], equal_nan=True), (k, what)       # (equal_nan: the arrow arrays of a call without norm terms are never written)


ITERATE = ('X1', 'X2', 'S1', 'S2', 'P', 'V', 'Hb', 'S1i', 'S2i', 'G', 'phi', 'z', 'at', 'aX', 'aSi', 'aLi', 'aLXi')


# ------------------------------------------------------------------------------------------------------------------------------ 1. state at the stop
def test_state_at_the_stop_points(case):
    """the phase the case is about, no lift and no frozen pivot; row K of the trace absent before s3 and present at s3; what iteration K does not write between two
    points is bit-identical across the four calls (the iterate and what k_phi_pre derives from it; pvec and the matrix part of psm from s0 on; the direction between
    s2 and s3); for K >= 2 the multipliers have left their starting values by more than 1e-2 relative"""
    K, kind, dm = case['K'], case['kind'], case['dm']
    b0 = case['solved'][0]
    assert len(members(case)) >= 1
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
            _bit_equal(g[0], g[i], ITERATE + ('pvec',), f's0 vs s{i}')
        gg = dm['nzs'] * dm['nzs'] + 2 * dm['nzs']
        assert np.array_equal(g[0]['psm'][:, :gg], g[2]['psm'][:, :gg])
        _bit_equal(g[1], g[2], ('corrp', 'acor'), 's1 vs s2: the Mehrotra terms are written in pass 1 only')
        _bit_equal(g[2], g[3], ('dphi', 'dz', 'adt', 'adX', 'asum', 'dP', 'eigmin'), 's2 vs s3')
        x0 = 1.0 / (dm['p'] * dm['n'])
        for s in stages(case, case['s0'], b):
            if s['m'] == 0:
                continue
            start = np.minimum(1.0, 1.0 / np.sum(s['G'] ** 2, axis=1))
            for e, a0, am in s['arrows']:
                start[a0:a0 + am] = min(1.0, x0 * np.sqrt(am) / wr_of(case, case['s0'], b))
            if K == 1:
                assert np.allclose(s['phi'], start, rtol=1e-14, atol=0), (s['k'], s['phi'], start)
                assert np.allclose(s['z'], x0 / start, rtol=1e-14, atol=0)
            else:
                assert np.linalg.norm(s['phi'] - start) > 1e-2 * np.linalg.norm(s['phi']), ('phi still at its starting value', s['k'])
    for b in range(dm['nb']):
        if b not in [m[0] for m in members(case)]:
            assert case['s3']['iprob'][b, I_PHASE] == PH_DONE


# ------------------------------------------------------------------------------------------------------------------------------ 2. k_phi_pre
def test_phi_pre_outputs(case):
    """pvec (w, u: m = n; V w, V u from the device w, u: m = n), c_tau (m = n), c_alpha (m = 2n + 2: n for Hb u, the product, n for the sum, the two cones), the Gram
    products where the handle keeps them in memory (m = n), T_loc,loc (from the device Gram products m = 8: four products, three sums, the half; from the device
    w, u the Gram products' own n each: 2n + 8; + z / phi: 2), the arrow entries from the device X and S^-1 (T[phi, phi]: m = 8 more; T[phi, t]: 2 ne + 3;
    T[t, t]: ne^2), the inverses of the arrow blocks by residual, and the partial sums Q_XS, Q_RPHI2, Q_NCONE"""
    dm = case['dm']
    n = dm['n']
    for b, phase, chord in members(case):
        snap = case['s0']
        wr = wr_of(case, snap, b)
        for s in stages(case, snap, b):
            k, m = s['k'], s['m']
            what = f'problem {b} stage {k}'
            w, u, wb, ub = ph.row_vectors(s['X'], s['Si'], s['G'])
            _inside(s['w'], w, wb, n, what + ' w'); _inside(s['u'], u, ub, n, what + ' u')
            Vw, Vu, Vwb, Vub = ph.row_images(snap['V'][b, k], s['w'], s['u'])
            _inside(s['Vw'], Vw, Vwb, n, what + ' V w'); _inside(s['Vu'], Vu, Vub, n, what + ' V u')
            ct, ca, ctb, cab = ph.border_entries(s['w'], s['u'], snap['Hb'][b, k])
            _inside(s['ct'][:m], ct, ctb, n, what + ' c_tau'); _inside(s['ca'][:m], ca, cab, 2 * n + 2, what + ' c_alpha')
            assert not s['ct'][m:].any() and not s['ca'][m:].any()
            GXG, GSG, GXb, GSb = ph.gram_products(s['G'], s['w'], s['u'])
            mT = 2 * n + 10
            if dm['prs']:
                prs = snap['prs'][b, k]
                dX, dS = prs[0:2, :m, :m], prs[2:4, :m, :m]
                _inside(dX, GXG, GXb, n, what + ' GXG'); _inside(dS, GSG, GSb, n, what + ' GSG')
                GXG, GSG, GXb, GSb, mT = np.asarray(dX, LD), np.asarray(dS, LD), np.abs(dX), np.abs(dS), 10
            T, _ = ph.rows_block(GXG, GSG, s['phi'], s['z'])
            Tb, _ = ph.rows_block(GXb, GSb, s['phi'], s['z'])
            res, resb = ph.rows_residual(GXG, s['z'])
            resb = ph.rows_residual(GXb, s['z'])[1]
            nz = s['nz']
            Tf = np.zeros((nz, nz), LD); Tfb = np.zeros((nz, nz), LD)
            Tf[:m, :m] = T; Tfb[:m, :m] = Tb
            mm = np.full((nz, nz), mT)
            res = np.concatenate([res, np.zeros(nz - m, LD)]); resb = np.concatenate([resb, np.zeros(nz - m, LD)])
            xs_arrows = []
            for e, a0, am in s['arrows']:
                ne = am + 1
                X, Si = s['aX', e], s['aSi', e]
                S = np.asarray(ph.arrow(s['at', e], s['phi'][a0:a0 + am], wr), float)
                xs_arrows.append((X, S))
                I = np.eye(ne, dtype=LD)
                # S^-1, L_S^-1, L_X^-1: residuals against the condition number, m = 3 ne as in test_inverses
                lim = 4 * sr.gamma(3 * ne)
                assert np.abs(np.asarray(S, LD) @ np.asarray(Si, LD) - I).max() <= lim * np.linalg.cond(S), (what, e, 'aSi')
                for name, mat in (('aLi', S), ('aLXi', X)):
                    Li = np.asarray(s[name, e], LD)
                    assert not np.triu(s[name, e], 1).any() and np.all(np.diagonal(s[name, e]) > 0), (what, e, name)
                    assert np.abs(Li @ np.asarray(mat, LD) @ Li.T - I).max() <= lim * np.linalg.cond(mat), (what, e, name)
                Tqq, Tqt, Ttt, Tqqb, Tqtb, Tttb = ph.arrow_schur(X, Si, wr)
                sl = slice(a0, a0 + am)
                Tf[sl, sl] += Tqq; Tfb[sl, sl] += Tqqb; mm[sl, sl] = mT + 9
                Tf[sl, m + e] = Tqt; Tf[m + e, sl] = Tqt; Tfb[sl, m + e] = Tqtb; Tfb[m + e, sl] = Tqtb; mm[sl, m + e] = mm[m + e, sl] = 2 * ne + 3
                Tf[m + e, m + e] = Ttt; Tfb[m + e, m + e] = Tttb; mm[m + e, m + e] = ne * ne
                rq, rt, rqb, rtb = ph.arrow_residual(X, wr)
                res[sl] += rq; resb[sl] += rqb; res[m + e] = rt; resb[m + e] = rtb
            for mv in np.unique(mm):
                sel = mm == mv
                _inside(np.where(sel, s['K'], 0.0), np.where(sel, Tf, 0), np.where(sel, Tfb, 0), int(mv), what + f' T_loc,loc (entries of m = {mv})')
            # partial sums.  Q_RPHI2 = sum r^2, r of m = n + 4 roundings with bound rb >= |r|: r^2 within (2 (n + 4) + 1) of rb^2, then nz terms
            part = snap['part'][b, k]
            _inside(np.array([part[Q_RPHI2]]), np.array([np.sum(res * res)]), np.array([np.sum(resb * resb)]), 2 * n + 9 + max(nz, 1), what + ' Q_RPHI2')
            assert part[Q_NCONE] == m + sum(am + 1 for _, _, am in s['arrows'])
            xs = [np.sum(np.asarray(snap[f'X{r}'][b, k], LD) * np.asarray(snap[f'S{r}'][b, k], LD)) for r in (1, 2)]
            xsb = [np.sum(np.abs(snap[f'X{r}'][b, k] * snap[f'S{r}'][b, k])) for r in (1, 2)]
            v, vb = ph.complementarity(s['phi'], s['z'], xs_arrows)
            _inside(np.array([part[Q_XS]]), np.array([xs[0] + xs[1] + v]), np.array([xsb[0] + xsb[1] + vb]),
                    2 * n * n + m + sum((am + 1) ** 2 for _, _, am in s['arrows']) + 2, what + ' Q_XS')


# ------------------------------------------------------------------------------------------------------------------------------ 3. k_aug_fill
def _coupling_slot(case, O, k, rows, d):
    """the rows `rows` (of block k+1) x the d columns of P_k of the coupling slot of stage k, whichever way it is stored"""
    return O[k][rows, :d] if case['orient'][k] == 0 else O[k][:d, rows].T


def test_aug_fill(case):
    """rows d .. d + nz - 1 of block k+1: b_k,i in the first d columns of D (a + b at p = 1), T_loc,loc in the lower triangle behind them and its diagonal in Ddiag
    (bit copies of psm), a_k,i in the same rows of the coupling slot of stage k in the orientation of the schedule; a, b from the device pvec with m = 6 (four
    products, their sum, the half; 7 with the sum a + b); the epigraph rows, the rows beyond d + nz and the other triangle of the slot untouched: identity, ones, zeros"""
    dm = case['dm']
    p, nx, d, dp = dm['p'], dm['nx'], dm['d'], dm['dp']
    for b, phase, chord in members(case):
        if chord:
            continue                                               # a chord step assembles nothing
        snap = case['s0']
        D, O, Dd = snap['D'][b], snap['O'][b], snap['Ddiag'][b]
        for s in stages(case, snap, b):
            k, kn, m, nz = s['k'], s['kn'], s['m'], s['nz']
            what = f'problem {b} stage {k}'
            rows = slice(d, d + m)
            a, bb, ab, bbb = ph.coupling_rows(s['w'], s['u'], s['Vw'], s['Vu'], nx)
            if p == 1:
                _inside(D[kn][rows, :d], a + bb, ab + bbb, 7, what + ' a + b in D')
            else:
                _inside(D[kn][rows, :d], bb, bbb, 6, what + ' b in D of block k+1')
                _inside(_coupling_slot(case, O, k, rows, d), a, ab, 6, what + ' a in the coupling slot')
            tail = D[kn][d:d + nz, d:d + nz]
            assert np.array_equal(np.tril(tail), np.tril(s['K'])), what + ': T_loc,loc in D'
            assert np.array_equal(Dd[kn][d:d + nz], np.diagonal(s['K'])), what + ': Ddiag'
            # untouched: the epigraph rows do not reach P; beyond d + nz the identity of k_schur; the slot's rows and columns beyond d except the a rows
            assert not D[kn][d + m:d + nz, :d].any(), what + ': epigraph rows reach P'
            assert np.array_equal(np.tril(D[kn])[d + nz:, :], np.eye(dp)[d + nz:, :]) and np.array_equal(Dd[kn][d + nz:], np.ones(dp - d - nz)), what + ': padding of D'
            Ok = O[k] if case['orient'][k] == 0 else O[k].T
            if p > 1:
                assert not Ok[d + m:, :].any() and not Ok[:, d:].any(), what + ': padding of the coupling slot'
            else:
                assert not Ok[d:, :].any() and not Ok[:, d:].any(), what + ': the coupling slot at p = 1'


# ------------------------------------------------------------------------------------------------------------------------------ 4. right-hand sides
def _r_loc(case, snap, b, s, sig, use_corr):
    """r_loc of one stage from the device T_r, G, phi, corrp, S^-1 and acor.   -> (value, bound, m per entry)"""
    n = case['dm']['n']
    wr = wr_of(case, snap, b)
    m, nz = s['m'], s['nz']
    r, rb = ph.rhs_rows(snap['T1'][b, s['k']], snap['T2'][b, s['k']], s['G'], s['phi'], sig, s['corrp'] if use_corr else None)
    r = np.concatenate([r, np.zeros(nz - m, LD)]); rb = np.concatenate([rb, np.zeros(nz - m, LD)])
    mm = np.full(nz, 2 * n + 5)                                    # T1 - T2 (1), n products, the product with g, n for the sum; sig / phi, its sum, corrp
    for e, a0, am in s['arrows']:
        rq, rt, rqb, rtb = ph.arrow_rhs(s['aSi', e], sig, wr, s['acor', e] if use_corr else None)
        r[a0:a0 + am] += rq; rb[a0:a0 + am] += rqb; mm[a0:a0 + am] += 5
        r[m + e] = rt; rb[m + e] = rtb; mm[m + e] = 2 * (am + 1) + 2
    return r, rb, int(mm.max()) if nz else 1


def test_pass1_right_hand_sides(case):
    """s0, main phase: r_loc of pass 1 in psm (sig = 0, no Mehrotra terms); the tails of W3 (r_loc | c_tau | c_alpha) and U (c_tau | c_alpha) of block k+1 bit
    copies of psm, zeros beyond d + nz.  (The assembled stop runs k_phi_rhs and k_aug_gather like the solver does.)"""
    dm = case['dm']
    d = dm['d']
    for b, phase, chord in members(case):
        if phase != PH_MAIN:
            continue
        snap = case['s0']
        for s in stages(case, snap, b):
            what = f'problem {b} stage {s["k"]}'
            r, rb, m = _r_loc(case, snap, b, s, 0.0, False)
            _inside(s['r'], r, rb, m, what + ' r_loc of pass 1')
            nz = s['nz']
            W3, U = snap['W3'][b, s['kn']], snap['U'][b, s['kn']]
            assert np.array_equal(W3[d:d + nz], np.stack([s['r'], s['ct'], s['ca']], axis=1)), what + ': W3 tail'
            assert np.array_equal(U[d:d + nz], np.stack([s['ct'], s['ca']], axis=1)), what + ': U tail'
            assert not W3[d + nz:].any() and not U[d + nz:].any(), what + ': padding of W3 / U'


def test_pass2_right_hand_sides(case):
    """s2: r_loc of pass 2 from the device T_r of pass 2: main phase sig = sigma mu with corrp and acor of pass 1; centering sig = mu_t WITHOUT them (they still hold
    the terms of the last main-phase iteration: a kernel that subtracted them would be found)"""
    for b, phase, chord in members(case):
        snap = case['s2']
        sig = snap['prob'][b][P_SIGMU]
        assert sig > 0.0
        for s in stages(case, snap, b):
            if phase != PH_MAIN and s['m']:
                assert s['corrp'].any()
            r, rb, m = _r_loc(case, snap, b, s, sig, phase == PH_MAIN)
            _inside(s['r'], r, rb, m, f'problem {b} stage {s["k"]} r_loc of pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 5. directions
def _directions(case, snap, b, pass1, phase, what):
    dm = case['dm']
    d = dm['d']
    pr = snap['prob'][b]
    wr = wr_of(case, snap, b)
    sig = 0.0 if pass1 else pr[P_SIGMU]
    use_corr = (not pass1) and phase == PH_MAIN
    for s in stages(case, snap, b):
        m, nz, kn = s['m'], s['nz'], s['kn']
        w_ = what + f' stage {s["k"]}'
        dy, dyb = ph.local_direction(snap['Z'][b, kn, d:d + nz], snap['TU'][b, kn, d:d + nz], pr[P_DTAU], pr[P_DALPHA])
        _inside(s['dphi'], dy[:m], dyb[:m], 4, w_ + ' dphi')                                   # m = 4: two products, two differences
        dz, dzb = ph.dual_direction(s['phi'], s['z'], s['dphi'], sig, s['corrp'] if use_corr else None)
        _inside(s['dz'], dz, dzb, 7, w_ + ' dz')                                               # two divisions, a product, three differences
        if pass1:
            v, vb = ph.mehrotra_rows(s['dz'], s['dphi'], s['phi'])
            _inside(s['corrp'], v, vb, 2, w_ + ' corrp')
        sums = np.zeros(3, LD); sumsb = np.zeros(3, LD)
        emd = emp = 0.0
        for e, a0, am in s['arrows']:
            ne = am + 1
            _inside(np.array([s['adt', e]]), dy[m + e:m + e + 1], dyb[m + e:m + e + 1], 4, w_ + f' dt of arrow {e}')
            S = ph.arrow(s['at', e], s['phi'][a0:a0 + am], wr)
            dS = ph.arrow(s['adt', e], s['dphi'][a0:a0 + am], wr)
            dS64 = np.asarray(dS, float)
            v, vb = ph.arrow_dX(s['aX', e], s['aSi', e], dS64, sig, s['acor', e] if use_corr else None)
            _inside(s['adX', e], v, vb, 2 * ne + 6, w_ + f' dX of arrow {e}')                   # w dphi (1), two nested sums of ne products, the half-sum, sig S^-1, three differences
            if pass1:
                v, vb = ph.arrow_corrector(s['adX', e], dS64, s['aSi', e])
                _inside(s['acor', e], v, vb, 2 * ne + 2, w_ + f' acor of arrow {e}')
                assert np.array_equal(s['acor', e], s['acor', e].T)
            v, vb = ph.arrow_sums(s['adX', e], np.asarray(S, float), s['aX', e], dS64)
            sums += v; sumsb += vb
            for name, mat, slot in (('aLi', dS64, 0), ('aLXi', s['adX', e], 1)):
                W = np.asarray(ph.step_matrix(s[name, e], mat)[0], float)
                ev = np.linalg.eigvalsh(W)
                if slot == 0:
                    emd = min(emd, ev[0])
                else:
                    emp = min(emp, ev[0])
                s['escale', e, slot] = np.abs(ev).max()
        asum = snap['asum'][b, s['k']]
        nsum = sum((am + 1) ** 2 for _, _, am in s['arrows']) + 2
        _inside(asum[:3], sums, sumsb, nsum, w_ + ' asum <dX,S>, <X,dS>, <dX,dS>')
        # smallest eigenvalues of the arrow step matrices (0 without arrows: the minimum starts there): 1e-12 of the matrix's scale, as for k_eigmin; the matrix
        # itself carries 2 ne + 1 roundings of entries up to cond * scale, absorbed by the same tolerance times the conditioning of L^-1
        for slot, ref in ((0, emd), (1, emp)):
            scale = max([s.get(('escale', e, slot), 0.0) for e, _, _ in s['arrows']] + [0.0])
            assert abs(asum[3 + slot] - ref) <= 1e-12 * scale, (w_, 'arrow eigenvalue', slot, asum[3 + slot], ref, scale)


def test_directions(case):
    """dphi, dt (the tail of the block solution, m = 4), dz (m = 7), corrp (pass 1, m = 2), the arrow dX (m = 2 ne + 6) and acor (pass 1, m = 2 ne + 2), the three sums
    and the two smallest eigenvalues of asum -- both passes, from the device Z, TU, dtau, dalpha, phi, z, X, S^-1, L^-1"""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _directions(case, case['s1'], b, True, phase, f'problem {b} pass 1')
        _directions(case, case['s2'], b, False, phase, f'problem {b} pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 6. local Newton rows
def _dense_system(case, b, phase):
    """the system assembled at s0 as one dense symmetric matrix [p dp + 2]: blocks D_k (lower triangles), coupling slots, border columns U and the 2 x 2 border.
    The main phase gathers U in pass 1 (at s0) and sums the border entries in its k_solve_border (s1); a centering iteration does both in pass 2 (s2)."""
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


def _local_rows_residual(case, b, Kd, rhs, x):
    """largest residual of the stage-local rows of Kd x = rhs relative to the largest term of those rows"""
    dm = case['dm']
    d, dp = dm['d'], dm['dp']
    worst = 0.0
    for s in stages(case, case['s0'], b):
        if s['nz'] == 0:
            continue
        rows = s['kn'] * dp + d + np.arange(s['nz'])
        res = Kd[rows] @ x - rhs[rows]
        scale = np.abs(Kd[rows]) @ np.abs(x) + np.abs(rhs[rows])
        worst = max(worst, float(np.max(np.abs(res) / scale)))
    return worst


def _device_solution(case, snap, b):
    dm = case['dm']
    p, d, dp, nx = dm['p'], dm['d'], dm['dp'], dm['nx']
    ia, ib = sr.tri_idx(nx)
    x = np.zeros(p * dp + 2)
    for k in range(p):
        x[k * dp:k * dp + d] = snap['dP'][b, k][ia, ib]
    for s in stages(case, snap, b):
        o = s['kn'] * dp + d
        x[o:o + s['m']] = s['dphi']
        for e, _, _ in s['arrows']:
            x[o + s['m'] + e] = s['adt', e]
    x[-2:] = snap['prob'][b][[P_DTAU, P_DALPHA]]
    return x


def local_newton_residuals(case, b, phase):
    """[(pass, device, reference)]: the residual of the stage-local rows T_loc,P dP + c_tau dtau + c_alpha dalpha + T_loc,loc dy = r_loc of the system assembled at s0,
    with the device direction and with the direction of a dense fp64 LAPACK solve of that system (floored at 2^-53)"""
    dm = case['dm']
    p, dp, nx = dm['p'], dm['dp'], dm['nx']
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
            r3[:, :dm['d']] = cols
            for s in stages(case, snap, b):
                r3[s['kn'], dm['d']:dm['d'] + s['nz']] = s['r']
            sig, corr0, part = pr[P_SIGMU], pr[P_CORR0], snap['part'][b]
        t0 = sig / pr[P_S0] - pr[P_X0] * pr[P_RD0] / pr[P_S0] - corr0
        rhs[N:] = [part[:, Q_TRT2].sum() - 1.0, part[:, Q_HBG].sum() + t0]
        ref = np.linalg.solve(Kd, rhs)
        out.append((pas, _local_rows_residual(case, b, Kd, rhs, _device_solution(case, snap, b)), max(_local_rows_residual(case, b, Kd, rhs, ref), 2.0 ** -53)))
    return out


def test_local_newton_rows(case):
    """The directions satisfy the stage-local rows of the Newton equations of the system the kernels assembled: ties k_aug_fill, k_aug_gather, the block solve, the
    border solve and k_phi_dir's tail read together.  The error of a solve has no rounding bound, so the device residual is held against that of a dense fp64 LAPACK
    solve of the same assembled system by LOCAL_NEWTON_FACTOR of its kind of step."""
    for b, phase, chord in members(case):
        if chord:
            continue
        kind = 'float32' if case['s2']['iprob'][b, I_LOWP] else ('fp64' if phase == PH_MAIN else 'center')
        for pas, dev, ref in local_newton_residuals(case, b, phase):
            print(f'local-newton-residual {_id((case["case"], case["kind"], case["generic"]))} problem {b} pass {pas} {kind}: device {dev:.3e} reference {ref:.3e} ratio {dev / ref:.3g}')
            assert ref <= 1e-6, (b, pas, ref)
            assert dev <= LOCAL_NEWTON_FACTOR[kind] * ref, (b, pas, kind, dev, ref, dev / ref)


# ------------------------------------------------------------------------------------------------------------------------------ 7. k_phi_steps
def _steps(case, snap, b, phase, pass2, what):
    dm = case['dm']
    n = dm['n']
    g = {k: v[b] for k, v in snap.items()}
    # the sums of the two LMIs (m = 2 n^2 + 1, as tests/test_gpu_step_kernels.py holds them), then the linear cone (m rows) and the arrow blocks (asum)
    X, S, dX, dS = ([np.asarray(g[a + r], LD) for r in '12'] for a in ('X', 'S', 'dX', 'dS'))
    f = lambda A, B, fn: sum(np.sum(fn(A[r] * B[r]), axis=(1, 2)) for r in (0, 1))
    v = np.stack([f(dX, S, lambda t: t), f(X, dS, lambda t: t), f(dX, dS, lambda t: t)], axis=1)
    vb = np.stack([f(dX, S, np.abs), f(X, dS, np.abs), f(dX, dS, np.abs)], axis=1)
    ev = np.linalg.eigvalsh(g['Wm'])
    th = eig_thresholds(phase)
    for s in stages(case, snap, b):
        k, m = s['k'], s['m']
        lv, lb = ph.linear_cone_sums(s['phi'], s['z'], s['dphi'], s['dz'])
        asum = g['asum'][k]
        for j, q in enumerate((Q_DXS, Q_XDS, Q_DXDS)):
            _inside(np.array([g['part'][k, q]]), np.array([v[k, j] + lv[j] + LD(asum[j])]), np.array([vb[k, j] + lb[j] + abs(LD(asum[j]))]), 2 * n * n + m + 3,
                    what + f' stage {k} partial sum {st.PART_NAMES[j]}')
        ls, lx = ph.linear_cone_steps(s['phi'], s['z'], s['dphi'], s['dz'])
        for slot, fold in ((0, min(ls, asum[3])), (1, min(lx, asum[4]))):
            got, ref, scale = g['eigmin'][k, slot], ev[k, slot, 0], np.abs(ev[k, slot]).max()
            if got == fold:
                # the LMI's own answer (its eigenvalue, or a bound -1 / theta below it) is not smaller than the folded value: neither is the eigenvalue
                assert ref >= fold - 1e-12 * scale, (what, k, slot, got, ref)
            else:
                # the LMI's own answer is smaller: the eigenvalue, or (pass 2 of k_eigmin) the bound -1 / theta of its pre-test
                assert got < fold, (what, k, slot, got, fold)
                assert abs(got - ref) <= 1e-12 * scale or (pass2 and any(got == -1.0 / t and ref > got for t in th)), (what, k, slot, got, ref)


def test_steps_fold(case):
    """what k_phi_steps folds into the step-length minima and the mu_aff sums: eigmin[0] = min(LMI 1's dual answer, min dphi / phi, arrows' dual minimum) and
    eigmin[1] likewise with dz / z -- the folded value is bit-exact in fp64 (a correctly rounded division and minima) -- and Q_DXS, Q_XDS, Q_DXDS = the two LMIs
    (m = 2 n^2 + 1) + the linear cone (m rows) + the device asum"""
    for b, phase, chord in members(case):
        if phase == PH_MAIN:
            _steps(case, case['s1'], b, phase, False, f'problem {b} pass 1')
        _steps(case, case['s2'], b, phase, True, f'problem {b} pass 2')


# ------------------------------------------------------------------------------------------------------------------------------ 8. k_phi_update
def test_update(case):
    """phi and t move by ad, z and the arrow X by ap (m = 2; the symmetrised X: 3), X exactly symmetric; some case has ap != ad (test_cases_tell_ap_from_ad); a member
    that left at the pre-check keeps its multipliers bit for bit"""
    dm = case['dm']
    for b, phase, chord in members(case):
        y = case['s3']
        ap, ad = y['prob'][b][P_AP], y['prob'][b][P_AD]
        assert ap > 0.0 and ad > 0.0
        for s2, s3 in zip(stages(case, case['s2'], b), stages(case, y, b)):
            what = f'problem {b} stage {s2["k"]}'
            for name, dname, a in (('phi', 'dphi', ad), ('z', 'dz', ap)):
                v, vb = ph.update(s2[name], s2[dname], a)
                _inside(s3[name], v, vb, 2, what + ' updated ' + name)
                assert s2['m'] == 0 or not np.array_equal(s3[name], s2[name])
            for e, _, _ in s2['arrows']:
                v, vb = ph.update(s2['at', e], s2['adt', e], ad)
                _inside(np.array([s3['at', e]]), np.array([v]), np.array([vb]), 2, what + f' updated t of arrow {e}')
                v, vb = ph.update(s2['aX', e], s2['adX', e], ap, symmetric=True)
                _inside(s3['aX', e], v, vb, 3, what + f' updated X of arrow {e}')
                assert np.array_equal(s3['aX', e], s3['aX', e].T)
    idle = [b for b in range(dm['nb']) if b not in [m[0] for m in members(case)]]
    for b in idle:
        for name in ('phi', 'z') + (('at', 'aX') if dm['arrows'] else ()):
            assert np.array_equal(case['s2'][name][b], case['s3'][name][b]) and np.array_equal(case['s0'][name][b], case['s3'][name][b]), (b, name)
    if dm['nb'] == 3:
        assert idle == [1]


# ------------------------------------------------------------------------------------------------------------------------------ 9. the forms agree bit for bit
STAGE_PRE = ('phi', 'z', 'w', 'u', 'Vw', 'Vu', 'K', 'ct', 'ca', 'r')
STAGE_DIR = ('dphi', 'dz', 'corrp')
ARROW_PRE, ARROW_DIR = ('at', 'aX', 'aSi', 'aLi', 'aLXi'), ('adt', 'adX', 'acor')


def _same_bits(ca, cb, snap, b, full):
    """what the kernels have written by stop point `snap`, entry by entry (the rows a stage does not have, the arrow blocks a call does not use and the upper triangle
    of D are never written); full: the direction and what follows it as well"""
    a, z = ca[snap], cb[snap]
    for sa, sz in zip(stages(ca, a, b), stages(cb, z, b)):
        names = STAGE_PRE + (STAGE_DIR if full else ()) + tuple((n, e) for n in ARROW_PRE + (ARROW_DIR if full else ()) for e, _, _ in sa['arrows'])
        for name in names:
            assert np.array_equal(sa[name], sz[name]), (snap, b, sa['k'], name)
    assert np.array_equal(np.tril(a['D'][b]), np.tril(z['D'][b])), (snap, b, 'D')
    for name in ('Ddiag', 'O', 'W3', 'U', 'X1', 'X2', 'S1', 'S2', 'P', 'S1i', 'S2i', 'T1', 'T2') + (('asum', 'eigmin', 'dP', 'Z', 'TU', 'prob') if full else ()):
        assert np.array_equal(a[name][b], z[name][b]), (snap, b, name)
    cols = [Q_XS, Q_RPHI2, Q_NCONE, Q_TRT2, Q_HBG] + ([Q_DXS, Q_XDS, Q_DXDS] if full else [])
    assert np.array_equal(a['part'][b][:, cols], z['part'][b][:, cols]), (snap, b, 'partial sums')


@pytest.mark.parametrize('prm', [q for q in MAIN_CASES if not q[2] and q[0] not in LARGE_CASES], ids=_id)
def test_generic_forms_return_the_same_bits(prm):
    """k_phi_pre<BIGN>, k_phi_rhs<BIGN>, kb_phi_dm + k_phi_dir<BIGN> at n <= 32: 'same arithmetic in the same order: both forms return the same bits'
    (tmpc_phi.h).  TMPC_DEBUG_FLAG_GENERIC_STAGE cannot show that: it also swaps the stage kernels, whose S^-1, T_r -- and already the scaling of H -- differ in the
    last bits, so the two runs never hand the multiplier kernels the same inputs (the generic fixtures above hold the <BIGN> forms to the rounding bounds
    instead).  TMPC_DEBUG_FLAG_GENERIC_ROWS swaps the multiplier kernels alone: then everything written by each stop point -- pvec, psm, the tails of D / O, the
    right-hand sides, the directions, the iterate after K iterations -- is the same bits."""
    tuned, rows = run_case(prm), run_case(prm, rows_generic=True)
    for b, phase, chord in members(tuned):
        _same_bits(tuned, rows, 's0', b, False)
        for snap in ('s1', 's2', 's3'):
            _same_bits(tuned, rows, snap, b, True)
        assert np.array_equal(tuned['s3']['iprob'][b], rows['s3']['iprob'][b])


def _twins(K):
    big = run_case((BIGR_CASE, K, False))
    twin = run_case((BIGR_CASE, K, False), nc_room=BIGR_TWIN_NC)
    assert big['dm']['prs'] and not twin['dm']['prs'] and big['dm']['dp'] == twin['dm']['dp']
    return big, twin


def test_more_than_32_rows_same_arithmetic_same_bits():
    """k_phi_pre<false, BIGR> (a handle with room for 2 + 31 rows: the per-row vectors stay in pvec, the Gram products in prs) against the same problem on a handle
    with room for 32 (LDS), from the same starting point (K = 1): what both forms compute by the same arithmetic -- w, u, V w, V u, c_tau, c_alpha, the arrow
    blocks' inverses -- is the same bits.  (Every layer of the BIGR form is held to its rounding bound by the fixtures of BIGR_CASE above.)"""
    big, twin = _twins(1)
    for b, phase, chord in members(big):
        for name in ('X1', 'X2', 'S1i', 'S2i', 'G'):
            assert np.array_equal(big['s0'][name][b][..., :twin['dm']['nr'], :] if name == 'G' else big['s0'][name][b], twin['s0'][name][b]), name
        for sa, sz in zip(stages(big, big['s0'], b), stages(twin, twin['s0'], b)):
            for name in ('phi', 'z', 'w', 'u', 'Vw', 'Vu', 'ct', 'ca') + tuple((a, e) for a in ('aSi', 'aLi', 'aLXi') for e, _, _ in sa['arrows']):
                assert np.array_equal(sa[name], sz[name]), (sa['k'], name)


def test_more_than_32_rows_returns_the_same_bits():
    """... and everything, at every K: the multiplier state, the per-row vectors, T_loc,loc, the right-hand sides, the directions and the iterate bit for bit.  The BIGR
    form forms each Gram product g_i . w_rj, g_i . u_rj in one lane instead of across the wave, but in the order of wave_sum (rounded products, the xor butterfly
    32, 16, .. 1).  (Before that it summed them as one serial fma chain: T_loc,loc differed by 3.4e-16 of its largest entry at the starting point and the iterates by
    up to 5e-14 after five iterations -- rounding level, but not the same bits.)"""
    for K in (1, 2, 5):
        big, twin = _twins(K)
        d = big['dm']['d']
        for b, phase, chord in members(big):
            for snap in ('s0', 's2', 's3'):
                a, z = big[snap], twin[snap]
                for sa, sz in zip(stages(big, a, b), stages(twin, z, b)):
                    for name in ('phi', 'z', 'dphi', 'dz', 'corrp', 'w', 'u', 'Vw', 'Vu', 'K', 'ct', 'ca', 'r'):
                        assert np.array_equal(sa[name], sz[name]), (K, snap, sa['k'], name)
                for name in ('X1', 'X2', 'S1', 'S2', 'P') + (('asum', 'eigmin', 'dP') if snap != 's0' else ()):      # (s0 of iteration 1: no direction written yet)
                    assert np.array_equal(a[name][b], z[name][b]), (K, snap, name)
            nzt = twin['dm']['nzs']
            assert np.array_equal(np.tril(big['s0']['D'][b][:, :d + nzt, :d + nzt]), np.tril(twin['s0']['D'][b][:, :d + nzt, :d + nzt]))


def test_cases_tell_ap_from_ad():
    """across the main-phase cases some step has ap != ad: test_update would not tell the two apart otherwise"""
    assert any(run_case(prm)['s3']['prob'][b][P_AP] != run_case(prm)['s3']['prob'][b][P_AD] for prm in MAIN_CASES if prm[0] not in LARGE_CASES
               for b, _, _ in members(run_case(prm)))
