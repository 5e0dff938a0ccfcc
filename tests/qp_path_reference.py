"""The PATH of the interior-point iterations of the MPC and periodic QP kernels (test infrastructure of test_qp_path_cpu.py / test_gpu_qp_path.py on top of
the six references, which state the iteration: mpc_qp_reference.ipm, ipm_soft, ipm_eq, ipm_quad, ipm_warm and periodic_qp_reference.ipm).

An interior-point method corrects itself: a wrong centring exponent, a wrong sign in the Mehrotra term or a term dropped from the corrector's right-hand side
still ends at the same point, a few iterations later.  The fixed point says nothing about them; the figures of the iterates do.  Both sides expose them
without a debug entry: `max_iter = k` ends the loop at iterate k with status 1 and the kernels write mu, rp, rd, pivmin of the last pass 1 into `info` at any
status, the references return mu, rp, rd the same way.  `path` makes the K calls.

Two classes of problems:
    'plain'  no equality or terminal rows.  The Newton system is solved twice: by plain fp64 LU (the references as they are) and by LU refined with longdouble
             residuals (`refined`: the better one, the truth of the GPU tests); the periodic family has a third, the staged elimination of the kernel
             (periodic_qp_reference.newton_staged);
    'eq'     equality or terminal rows at the weight 1 / RHO = 1e12.  The references form Je' Je / RHO and dnu = (Je dv + req) / RHO, a difference of two
             numbers blown up by 1e12: their own path is only good to 1e-5 .. 1e-4.  The truth is the augmented system (`augmented=True`: dnu an unknown, the
             block -RHO I, no 1 / RHO in the matrix), refined likewise.  The kernels eliminate stage by stage at the weight 1 / RHO, as the references do.
The comparison of a figure f (mu, rp, rd, pivmin) with the truth is  |f - f_ref| <= REL[class] f_ref + ABS[class];  the constants are 100 times the largest
spread between the two means on the CPU (test_qp_path_cpu.py measures it, profiles/qp_path_spread.txt records it), rounded up to one digit: 100 because the
error compounds over k steps and the device sums in another order.

r_d of the MPC families is restated with the scale of the rule and of the kernel (`stagewise_rd`): the references divide by max|g| of the dense problem.
The path cases are the small cases of the references plus three new ones (rows beyond one pass of the workgroup, nu > nx, periodic equality rows at every
phase over two periods), each at an instance whose stop test is decided by a factor 2.  The cases with equality rows are the quiet ones: the noise of the
weight 1 / RHO grows with the equality residual of the start, and periodic case_ragged / case_odd (five times the spread of the class) serve the stall
test of test_qp_path_cpu.py only.

`mutant` and `step_back` state the mutations of the reference that the comparison must see (centring exponent 2, the sign of the ds dl term, STEP_BACK 0.99)."""
import contextlib
import types

import numpy as np
import scipy.linalg as sla

import lqr_ctg_reference as lc
import mpc_qp_reference as mq
import mpc_qp_soft_reference as ms
import mpc_qp_eq_reference as eqr
import mpc_qp_affine_reference as afr
import mpc_qp_quad_reference as mqq
import mpc_qp_warm_reference as wr
import periodic_qp_reference as pq

FIGURES = ('mu', 'rp', 'rd')
# The spread of a figure above SPLIT is measured relatively, of one below it absolutely: a residual that has reached rounding has an absolute spread, and so
# has the dual residual of the class 'eq' below 1e-2 (the noise of the weight 1 / RHO is 1e-4 of the equality residual of the step before).
SPLIT = {'plain': 1e-6, 'eq': 1e-2}
# 100 x the largest spread of test_qp_path_cpu.py (profiles/qp_path_spread.txt), rounded up to one digit.
REL = {'plain': 3e-7, 'eq': 7e-2}
ABS = {'plain': 3e-12, 'eq': 6e-4}
MARGIN = 100.0


def path(ipm_fn, *args, K, rd_of=None, **kw):
    """ipm_fn(*args, max_iter=k, **kw) for k = 0 .. K -> dict of arrays [K + 1]: status, iters, mu, rp, rd, lmax (max lam of the iterate; 0 without rows) and
    pivmin where the iteration returns it.  Entry k is iterate k, or the converged iterate once k reaches its number.  rd_of: a function of the returned
    dict that restates r_d (stagewise_rd)."""
    out = dict(status=np.zeros(K + 1, int), iters=np.zeros(K + 1, int), mu=np.zeros(K + 1), rp=np.zeros(K + 1), rd=np.zeros(K + 1), lmax=np.zeros(K + 1),
               pivmin=np.full(K + 1, np.nan))
    for k in range(K + 1):
        a = ipm_fn(*args, max_iter=k, **kw)
        out['status'][k], out['iters'][k] = a['status'], a['iters']
        for f in FIGURES:
            out[f][k] = a[f]
        if rd_of is not None:
            out['rd'][k] = rd_of(a)
        out['lmax'][k] = a['lam'].max() if len(a['lam']) else 0.0
        out['pivmin'][k] = a.get('pivmin', np.nan)
    return out


def count_of(ipm_fn, *args, **kw):
    """The iteration count of the converged run."""
    a = ipm_fn(*args, **kw)
    assert a['status'] == 0, a['status']
    return int(a['iters'])


# ----------------------------------------------------------------------------- the better linear algebra
def refined_solve(A, b):
    """A x = b by fp64 LU with partial pivoting, refined with residuals in longdouble until the correction is below one ulp of x (the way cr_reference
    measures its residuals): x is the fp64 rounding of the solution while cond(A) stays below 1 / eps."""
    A = np.asarray(A, float); b = np.asarray(b, float)
    lu = sla.lu_factor(A)
    x = sla.lu_solve(lu, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    xl = x.astype(np.longdouble)
    for _ in range(6):
        dx = sla.lu_solve(lu, (bl - Al @ xl).astype(float))
        xl = xl + dx
        if np.abs(dx).max() <= 2.0 ** -54 * np.abs(xl).max():
            break
    return xl.astype(float)


class _Linalg:
    solve = staticmethod(refined_solve)

    def __getattr__(self, k):
        return getattr(np.linalg, k)


class _Numpy:
    linalg = _Linalg()

    def __getattr__(self, k):
        return getattr(np, k)


@contextlib.contextmanager
def refined(*modules):
    """Inside the block every np.linalg.solve of the given reference modules is refined_solve.  Nothing else of them changes, so the iteration is the one
    they state; the modules are restored on exit."""
    saved = [m.np for m in modules]
    for m in modules:
        m.np = _Numpy()
    try:
        yield
    finally:
        for m, s in zip(modules, saved):
            m.np = s


# ----------------------------------------------------------------------------- mutations of the references
def mutant(module, *pairs):
    """A copy of a reference module with each (old, new) of `pairs` replaced in its text; every `old` must occur exactly once."""
    import inspect
    src = inspect.getsource(module)
    for old, new in pairs:
        assert src.count(old) == 1, (module.__name__, old, src.count(old))
        src = src.replace(old, new)
    m = types.ModuleType(module.__name__ + '_mutant')
    m.__file__ = module.__file__
    exec(compile(src, module.__file__, 'exec'), m.__dict__)
    return m


@contextlib.contextmanager
def step_back(value):
    """mpc_qp_reference.STEP_BACK, which every reference reads, set to `value` inside the block."""
    saved = mq.STEP_BACK
    mq.STEP_BACK = value
    try:
        yield
    finally:
        mq.STEP_BACK = saved


EXPONENT = ('** 3', '** 2')
SIGN = {'hard': ('sigma * mu - ds * dl', 'sigma * mu + ds * dl')}            # the other references write it with sigmu
SIGN_DEFAULT = ('sigmu - ds * dl', 'sigmu + ds * dl')
MUTATIONS = ('exponent 2', 'STEP_BACK 0.99', 'sign of ds dl')


# ----------------------------------------------------------------------------- the comparison
def deviation(f, fref, cls):
    """-> (relative deviation where fref > SPLIT of the class, else 0; absolute deviation where fref <= SPLIT, else 0), elementwise."""
    f, fref = np.asarray(f, float), np.asarray(fref, float)
    big = fref > SPLIT[cls]
    d = np.abs(f - fref)
    return np.where(big, d / np.where(big, fref, 1.0), 0.0), np.where(big, 0.0, d)


def excess(f, fref, cls):
    """|f - fref| / (REL fref + ABS), elementwise: within the tolerance of the class when <= 1."""
    f, fref = np.asarray(f, float), np.asarray(fref, float)
    return np.abs(f - fref) / (REL[cls] * np.abs(fref) + ABS[cls])


def round_up(x):
    """x rounded up to one significant digit."""
    if x <= 0:
        return 0.0
    e = np.floor(np.log10(x))
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


def stop_ratio(pt, k, tol=mq.TOL):
    """The deciding figure of the stop test at iterate k of a path, as a multiple of its threshold: the test passes when <= 1."""
    return max(pt['rp'][k] / tol, pt['rd'][k] / tol, pt['mu'][k] / (mq.MU_FACTOR * tol * max(1.0, pt['lmax'][k])))


# ----------------------------------------------------------------------------- the MPC families: cases in the form of mpc_qp_warm_reference.problems()
_CACHE = {}
MPC_IPM = {'hard': (mq, 'ipm'), 'soft': (ms, 'ipm_soft'), 'eq': (eqr, 'ipm_eq'), 'affine': (eqr, 'ipm_eq'), 'quad': (mqq, 'ipm_quad'), 'warm': (wr, 'ipm_warm')}
MODULES = (mq, ms, eqr, mqq, wr, pq)


def case_many_rows():
    """Rows beyond one pass of the workgroup: p 3 / nx 2 / nu 1, N = 3 from phase 0, nd = 300 > 256 rows at phase 1 alone, unit rows on [x; u] placed
    around the solution without rows: rows 0 and 150 0.2 inside it (active), the others 0.5 beyond it."""
    if 'many_rows' not in _CACHE:
        A, B, Hc, _ = lc.gen_problem(202, 1, 3, 2, 1, 0)
        nd, p, n, N = 300, 3, 3, 3
        rng = np.random.default_rng(202)
        X0 = rng.standard_normal((1, 2, 2))
        Pf = np.ascontiguousarray(np.broadcast_to(np.eye(2), (1, p, 2, 2)))
        D = np.zeros((1, p, nd, n)); d = np.zeros((1, p, nd))
        Dk = rng.standard_normal((nd, n))
        D[0, 1] = Dk / np.linalg.norm(Dk, axis=1, keepdims=True)
        P = mq.dense(A[0], B[0], Hc[0], N, 0, X0[0, 0], Pf=Pf[0])
        Xf, Uf, _ = mq.unpack(P, mq.polish(P, np.zeros(0, bool))['v'])
        z1 = np.concatenate([Xf[1], Uf[1]])
        d[0, 1] = D[0, 1] @ z1 + np.where(np.arange(nd) % 150 == 0, -0.2, 0.5)
        _CACHE['many_rows'] = dict(A=A, B=B, H=Hc, Pf=Pf, X0=X0[:, :1], N=N, k0=0, q=None, D=D, d=d, rows=np.array([[0, nd, 0]]))
    return _CACHE['many_rows']


def case_more_inputs_than_states():
    """nu > nx: p 2 / nx 1 / nu 3, N = 3 from phase 1, the input box at half the largest unconstrained |u_0|."""
    if 'nu3_base' not in _CACHE:
        A, B, Hc, _ = lc.gen_problem(207, 1, 2, 1, 3, 0)
        _CACHE['nu3_base'] = dict(A=A, B=B, Hc=Hc)
    return mq._finish('path_nu3', _CACHE['nu3_base'], 3, 1, 2, 204, box=0.5)


def case_affine_edge():
    """The layout edge nx 40 / nu 24 (n = 64), N = 2, with its 4 rows per stage, an offset of scale 0.1 and qf of scale 0.5, no equality or terminal rows."""
    return afr._affine('path_aff_edge', eqr._case('path_edge_plain', mq.case_layout_edge(), 1.0), 61, c_scale=0.1, qf_scale=0.5)


HARD_KEYS = ('q', 'Pf', 'D', 'd', 'ndcnt')
EQ_KEYS = HARD_KEYS + ('penalty', 'J', 'r', 'necnt', 'terminal', 'offset', 'qf', 'terminal_rhs')


def _one(b, keys, s):
    """Instance s of the batch arguments b (nb = 1) as a problem in the form of mpc_qp_warm_reference.problems() with ns = 1."""
    return dict(A=b['A'], B=b['B'], H=b['H'], X0=np.ascontiguousarray(b['X0'][:, s:s + 1]), N=b['N'], k0=b['k0'], opt={k: b[k] for k in keys if b.get(k) is not None})


def _hard(c, s):
    return _one(dict(c, ndcnt=wr._i32(c['rows'])), HARD_KEYS, s)


def mpc_cases():
    """-> list of dict name, fam, cls, pr (the problem in the form of mpc_qp_warm_reference.problems(), nb = ns = 1).  The instance of each case is one whose
    stop test is decided by a factor 2 (test_qp_path_cpu.py asserts it in the class 'plain')."""
    if 'mpc' in _CACHE:
        return _CACHE['mpc']
    out = []
    add = lambda name, fam, cls, pr, **kw: out.append(dict(name=name, fam=fam, cls=cls, pr=pr, **kw))
    add('mixed_small', 'hard', 'plain', _hard(mq.case_mixed_small(), 1))
    add('box_nu2', 'hard', 'plain', _hard(mq.case_box_nu2(), 1))
    add('layout_edge', 'hard', 'plain', _hard(mq.case_layout_edge(), 0))
    add('many_rows', 'hard', 'plain', _hard(case_many_rows(), 0))
    add('more_inputs', 'hard', 'plain', _hard(case_more_inputs_than_states(), 0))
    skeys = HARD_KEYS + ('penalty',)
    add('box_nu1_f0.3', 'soft', 'plain', _one(ms.batch_of(ms.instances(mq.case_box_nu1, 0.3)[:1]), skeys, 0))
    add('mixed_small_f0.3', 'soft', 'plain', _one(ms.batch_of(ms.instances(mq.case_mixed_small, 0.3)[:1]), skeys, 0))
    add('layout_edge_f10', 'soft', 'plain', _one(ms.batch_of(ms.instances(mq.case_layout_edge, 10.0)[:1]), skeys, 0))      # n = 64 = LQR_NMAX
    add('term_p1', 'eq', 'eq', _one(eqr.batch_of(eqr.case_term_p1()), EQ_KEYS, 1))
    add('rows_mixed_small_N2', 'eq', 'eq', _one(eqr.batch_of(eqr.case_rows_mixed_small_N2()), EQ_KEYS, 0))
    add('aff_qf_box_nu1', 'affine', 'plain', _one(afr.batch_of(afr.case_aff_qf_box_nu1()), EQ_KEYS, 0))
    add('aff_edge', 'affine', 'plain', _one(afr.batch_of(case_affine_edge()), EQ_KEYS, 0))
    add('shift_term_p1', 'affine', 'eq', _one(afr.batch_of(afr.case_shift_term_p1()), EQ_KEYS, 1))
    qkeys = skeys + ('penalty2',)
    add('l12_box_nu1', 'quad', 'plain', _one(mqq.batch_of(mqq.instances('l12', mq.case_box_nu1, 0.3, 1.0)[:1]), qkeys, 0))
    add('pure_mixed_small', 'quad', 'plain', _one(mqq.batch_of(mqq.instances('pure', mq.case_mixed_small, 1e2)[:1]), qkeys, 0))
    _CACHE['mpc'] = out
    return out


def warm_case():
    """The warm family: mixed_small, instance 1, with the converged iterate of instance 3 as the guess for the same phase (guess_shift = 0)
    -> dict name, fam 'warm', cls, pr, guess (stage-wise, the keys of solve_warm), start (the floored start of ipm_warm)."""
    if 'warm' not in _CACHE:
        c = mq.case_mixed_small()
        pr, other = _hard(c, 1), _hard(c, 3)
        case = dict(name='mixed_small_guess', fam='warm', cls='plain', pr=pr)
        Po, cv, zv, _ = mpc_problem(dict(pr=other))
        a = wr.ipm_warm(Po, cv, zv)
        assert a['status'] == 0
        guess = wr.stagewise(Po, a)
        P, cvec, zvec, kw = mpc_problem(case)
        g = wr.shift_guess(guess, pr['X0'][0, 0], pr['A'][0], pr['B'][0], pr['k0'], kw.get('offset'), 0)
        case.update(guess=guess, start=wr.warm_start(P, cvec, zvec, g))
        _CACHE['warm'] = case
    return _CACHE['warm']


def mpc_problem(c):
    """-> (P, cvec, zvec, kw): the dense problem of the walked instance, its row weights and the keyword arguments of solve_warm / truth."""
    pr = c['pr']
    kw = wr.member_kw(pr, 0)
    P = wr.dense_of(pr['A'][0], pr['B'][0], pr['H'][0], pr['N'], pr['k0'], pr['X0'][0, 0], kw)
    cvec, zvec = wr.weights(P, pr['k0'], kw.get('penalty'), kw.get('penalty2'))
    return P, cvec, zvec, kw


def stagewise_rd(P, kw, a):
    """r_d of an iterate with the scale the rule states and the kernel uses, max(1, max_j |H z_j + q + D' lam_j + J' nu_j|) over the stages j = 0 .. N-1 and
    ALL their rows.  The MPC references take max|g| of the dense problem instead, which has no x rows at stage 0 (x_0 is data) and has the rows of x_N
    (Pf x_N + qf): the same numerator over another scale, a factor of 3 apart on a case with a large x_0.  (Their stop test keeps their scale; the cases
    are chosen so that either scale decides the same count: test_qp_path_cpu.py.)"""
    Q, c, G = P['Q'], P['c'], P['G']
    N, nx, mb, x0 = P['N'], P['nx'], P['mb'], P['x0']
    v, lam = a['v'], a['lam']
    nue = a.get('nue', np.zeros(0))
    Je = P.get('Je', np.zeros((0, len(c))))
    Js = np.where((P['escale'] == 0.0)[:, None], 0.0, Je) if len(Je) else Je
    gs = Q @ v + c + G.T @ lam + (Js.T @ nue if len(Je) else 0.0)
    num = a['rd'] * max(1.0, np.abs(gs).max())
    k0 = kw['k0']
    H0 = 0.5 * (kw['H'][k0] + kw['H'][k0].T)
    g0 = (H0 @ np.concatenate([x0, v[:mb]]))[:nx] + (0.0 if kw.get('q') is None else kw['q'][k0][:nx])
    _, _, Lam = mq.unpack(P, v, lam)
    if kw.get('D') is not None:
        m0 = int(kw['D'].shape[1] if kw.get('rows') is None else kw['rows'][k0])
        g0 = g0 + kw['D'][k0][:m0, :nx].T @ Lam[0, :m0]
    if kw.get('J') is not None:
        e0 = int(kw['J'].shape[1] if kw.get('erows') is None else kw['erows'][k0])
        g0 = g0 + kw['J'][k0][:e0, :nx].T @ eqr.unpack_nu(P, nue)[0][0, :e0]
    return num / max(1.0, np.abs(gs[:N * mb + (N - 1) * nx]).max(), np.abs(g0).max())


def mpc_ipm(fam, P, cvec, zvec, module=None, start=None, **kw):
    """The family's own iteration on a dense problem (module: a mutant of its reference module)."""
    mod, name = MPC_IPM[fam]
    f = getattr(module or mod, name)
    if fam == 'hard':
        return f(P, **kw)
    if fam == 'quad':
        return f(P, cvec, zvec, **kw)
    if fam == 'warm':
        return f(P, cvec, zvec, start, **kw)
    return f(P, cvec, **kw)


def mpc_walk(c, means='truth', module=None, K=None, start=None):
    """The path of a case by one of the means 'plain' (the reference as it is) or 'truth' (refined; augmented and refined in the class 'eq') -> (path, count);
    K defaults to the count of the plain reference + 1."""
    P, cvec, zvec, pkw = mpc_problem(c)
    pkw = dict(pkw, k0=c['pr']['k0'], H=c['pr']['H'][0])
    rd_of = lambda a: stagewise_rd(P, pkw, a)
    fam = c['fam']
    start = c.get('start') if start is None else start
    kw = dict(module=module, start=start)
    if K is None:
        K = count_of(lambda **k: mpc_ipm(fam, P, cvec, zvec, start=start, **k)) + 1
    if means == 'truth' and c['cls'] == 'eq':
        kw['augmented'] = True
    run = lambda **k: mpc_ipm(fam, P, cvec, zvec, **kw, **k)
    if means == 'truth':
        with refined(*MODULES, *([module] if module else [])):
            pt = path(run, K=K, rd_of=rd_of)
    else:
        pt = path(run, K=K, rd_of=rd_of)
    conv = np.flatnonzero(pt['status'] == 0)
    return pt, (int(conv[0]) if len(conv) else None)


def mpc_paths(c):
    """Both paths of a case, once per process -> dict plain, truth, n_plain, n_truth, K."""
    key = ('paths', c['fam'], c['name'])
    if key not in _CACHE:
        plain, n_plain = mpc_walk(c, 'plain')
        K = len(plain['mu']) - 1
        truth, n_truth = mpc_walk(c, 'truth', K=K)
        _CACHE[key] = dict(plain=plain, truth=truth, n_plain=n_plain, n_truth=n_truth, K=K)
    return _CACHE[key]


def mpc_certificate(c):
    """(a) then (b) of the family's reference on the walked instance -> (status of (a), certificate of (b), number of active rows)."""
    pr = c['pr']
    _, _, _, kw = mpc_problem(c)
    _, r = wr.truth(pr['A'][0], pr['B'][0], pr['H'][0], pr['N'], pr['k0'], pr['X0'][0, 0], **kw)
    return r['a']['status'], r['b']['certificate'], r['b']['nact']


def mpc_mutant_walk(c, which, K=3):
    """The truth-means path of a mutated reference over the first K iterates."""
    fam = c['fam']
    mod = MPC_IPM[fam][0]
    if which == 'STEP_BACK 0.99':
        with step_back(0.99):
            return mpc_walk(c, 'truth', K=K)[0]
    pair = EXPONENT if which == 'exponent 2' else SIGN.get(fam, SIGN_DEFAULT)
    return mpc_walk(c, 'truth', module=mutant(mod, pair), K=K)[0]


# ----------------------------------------------------------------------------- the periodic family
def case_periodic_many_rows():
    """p 2 / nx 2 / nu 1 with nd = 300 > 256 rows at phase 0 (two of them active) and none at phase 1."""
    def make():
        A, B, H, q, c = pq._model(60, 2, 1, 2)
        return A, B, H, 1, pq._rows(61, A, B, H, q, c, [300, 0], [0, 0], every=150)
    return pq._case('path_many_rows', make)


def case_periodic_more_inputs():
    """nu > nx: p 2 / nx 1 / nu 3 with the input box at 0.6 of the free orbit's largest input."""
    def make():
        A, B, H, q, c = pq._model(58, 1, 3, 2)
        return A, B, H, 1, pq._box(A, B, H, q, c, 0.6)
    return pq._case('path_more_inputs', make)


def case_periodic_rows_everywhere():
    """p 3 / nx 3 / nu 2 over two periods with equality rows at every phase (1 / 1 / 1) and inequality rows 2 / 1 / 2."""
    def make():
        A, B, H, q, c = pq._model(60, 3, 2, 3)
        return A, B, H, 2, pq._rows(61, A, B, H, q, c, [2, 1, 2], [1, 1, 1])
    return pq._case('path_rows_everywhere', make)


def periodic_cases():
    """-> list of dict name, fam 'periodic', cls, c (the case of periodic_qp_reference)."""
    mk = lambda f, cls: dict(name=f.__name__[5:], fam='periodic', cls=cls, c=f())
    return [mk(pq.case_scalar_bound, 'plain'), mk(pq.case_unstable, 'plain'), mk(pq.case_stage_shape, 'plain'), mk(case_periodic_many_rows, 'plain'),
            mk(case_periodic_more_inputs, 'plain'), mk(case_periodic_rows_everywhere, 'eq')]


def stall_cases():
    """The cases with equality rows on which the staged restatement was seen to stall (not path cases: their own spread is the largest of the class)."""
    return [dict(name=f.__name__[5:], fam='periodic', cls='eq', c=f()) for f in (pq.case_ragged, pq.case_odd)] + [periodic_cases()[-1]]


def periodic_problem(c):
    key = ('P', c['name'])
    if key not in _CACHE:
        cc = c['c']
        _CACHE[key] = pq.dense(cc['A'], cc['B'], cc['H'], cc['periods'], **cc['kw'])
    return _CACHE[key]


def periodic_walk(c, means='truth', module=None, K=None):
    """The path of a periodic case by 'plain' (newton_dense as it is), 'staged' (the kernel's elimination, plain fp64), 'recomputed' (the same with the row
    residuals evaluated again: newton_staged(reuse=False)) or 'truth' -> (path, count); every
    path carries pivmin, the pivots of the staged elimination at its own iterates."""
    P = periodic_problem(c)
    ipm = (module or pq).ipm
    if K is None:
        K = count_of(lambda **k: pq.ipm(P, **k)) + 1
    kw = dict(pivots=True)
    if means in ('staged', 'recomputed'):
        kw.update(staged=True, reuse=means == 'staged')
    if means == 'truth':
        kw['augmented'] = c['cls'] == 'eq'
        with refined(*MODULES, *([module] if module else [])):
            pt = path(ipm, P, K=K, **kw)
    else:
        pt = path(ipm, P, K=K, **kw)
    conv = np.flatnonzero(pt['status'] == 0)
    return pt, (int(conv[0]) if len(conv) else None)


def periodic_paths(c):
    """-> dict plain, staged, truth, n_plain, n_staged, n_truth, K, once per process."""
    key = ('paths', 'periodic', c['name'])
    if key not in _CACHE:
        plain, n_plain = periodic_walk(c, 'plain')
        K = len(plain['mu']) - 1
        staged, n_staged = periodic_walk(c, 'staged', K=K)
        truth, n_truth = periodic_walk(c, 'truth', K=K)
        _CACHE[key] = dict(plain=plain, staged=staged, truth=truth, n_plain=n_plain, n_staged=n_staged, n_truth=n_truth, K=K)
    return _CACHE[key]


def periodic_mutant_walk(c, which, K=3):
    if which == 'STEP_BACK 0.99':
        with step_back(0.99):
            return periodic_walk(c, 'truth', K=K)[0]
    return periodic_walk(c, 'truth', module=mutant(pq, EXPONENT if which == 'exponent 2' else SIGN_DEFAULT), K=K)[0]
