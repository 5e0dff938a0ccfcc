"""The two small shapes and the raw ctypes caller of test_mpc_qp_entries_cpu.py / test_gpu_mpc_qp_entries.py: the eight C entries tmpc_mpc_qp_*_batch_{host,device}
called as a C program would call them, with output buffers that tunempc_amd._lib never passes (Eol / nviol without penalty, optional outputs left out).

A problem is a dict: the sizes nb, p, nx, mb, nd, N, ns, T, k0, ne, nt, the arrays A, B, H, q, Pf, D, ndcnt, d, X0, penalty, J, r, necnt, Tx and aff (None or the
seven arrays offset, qf, terminal_rhs, Ap, Bp, cp, W), None where absent.  Nothing here is written to after it is built."""
import ctypes as C

import numpy as np

import mpc_qp_eq_reference as eq

LEVELS = ('hard', 'soft', 'eq', 'aff')
WHERE = ('host', 'device')
PREFIX = {'hard': '', 'soft': 'soft_', 'eq': 'eq_', 'aff': 'aff_'}
REQUIRED = ('U0', 'XT', 'info')
OPTIONAL = ('X', 'U', 'iters', 'nact', 'hres', 'Xol', 'Uol', 'Lam')
TAIL_OUT = {'hard': (), 'soft': ('Eol', 'nviol'), 'eq': ('Eol', 'nviol', 'Nu', 'NuT', 'eres'), 'aff': ('Eol', 'nviol', 'Nu', 'NuT', 'eres')}
ABSENT = dict(q=None, penalty=None, ne=0, J=None, r=None, necnt=None, nt=0, Tx=None, aff=None)


def symbol(level, where):
    return 'tmpc_mpc_qp_%sbatch_%s' % (PREFIX[level], where)


def shape_a(x0s=(-2.0, 0.1, 1.2)):
    """The scalar box problem of test_gpu_mpc_qp_eq.scalar_batch without its terminal constraint: nb = p = nx = nu = 1, nd = 2 (|u| <= 0.6), N = 2; ns = 3,
    T = 3.  The box is on the input alone, so every instance is feasible; the outer two states saturate the input at the first steps (the references say both
    in test_mpc_qp_entries_cpu.py)."""
    D = np.array([[[[0.0, 1.0], [0.0, -1.0]]]])
    return dict(ABSENT, nb=1, p=1, nx=1, mb=1, nd=2, N=2, ns=len(x0s), T=3, k0=0, A=np.array([[[[0.9]]]]), B=np.array([[[[0.7]]]]),
                H=np.array([[[[2.0, 0.3], [0.3, 1.5]]]]), Pf=np.array([[[[1.2]]]]), D=D, ndcnt=None, d=np.full((1, 1, 2), 0.6),
                X0=np.asarray(x0s, float).reshape(1, -1, 1))


def shape_b():
    """nb = 2, p = 2, nx = 2, nu = 1, nd = 2 with ndcnt [[2, 0], [0, 1]], N = 3, ns = 2, T = 2 from phase 1: mpc_qp_eq_reference.case_rows_mixed_small reduced to
    its first two states and its first input; problem 0 takes the phases 0, 1 of that case and problem 1 the phases 1, 2.  The equality rows (shape_b_rows:
    ne = 1, necnt [[1, 0], [0, 1]]) are the case's rows under the same reduction."""
    c = eq.case_rows_mixed_small()
    x, u, z = [0, 1], [0], [0, 1, 3]
    sub = lambda M, rows, cols: np.ascontiguousarray(_two_problems(M)[:, :, rows][:, :, :, cols])
    X0 = np.ascontiguousarray(np.stack([0.3 * c['X0'][0, :2, :2], 0.1 * c['X0'][0, 2:4, :2]]))
    return dict(ABSENT, nb=2, p=2, nx=2, mb=1, nd=2, N=3, ns=2, T=2, k0=1, A=sub(c['A'], x, x), B=sub(c['B'], x, u), H=sub(c['H'], z, z),
                q=np.ascontiguousarray(_two_problems(c['q'])[:, :, z]), Pf=np.ascontiguousarray(np.broadcast_to(np.eye(2), (2, 2, 2, 2))), D=sub(c['D'], [0, 1], z),
                ndcnt=np.array([[2, 0], [0, 1]], np.int32), d=_two_problems(c['d']), X0=X0)


def _two_problems(M):
    """An array [1, 3 phases, ...] of the case -> [2, 2 phases, ...]: the phases 0, 1 and 1, 2."""
    return np.ascontiguousarray(np.stack([M[0, [0, 1]], M[0, [1, 2]]]))


def shape_b_rows():
    c = eq.case_rows_mixed_small()
    return dict(ne=1, J=np.ascontiguousarray(_two_problems(c['J'])[:, :, :, [0, 1, 3]]), r=_two_problems(c['r']), necnt=np.array([[1, 0], [0, 1]], np.int32))


def shape_b_affine(P, rhs):
    """offset, qf, a disturbance (and with rhs a terminal right-hand side) for a problem of shape (b); the plant stays the model."""
    rng = np.random.default_rng(31)
    nb, p, nx, ns, T = (P[k] for k in ('nb', 'p', 'nx', 'ns', 'T'))
    t = 0.02 * rng.standard_normal((nb, p, nx)) if rhs else None
    return (0.05 * rng.standard_normal((nb, p, nx)), 0.1 * rng.standard_normal((nb, p, nx)), t, None, None, None, 0.01 * rng.standard_normal((nb, ns, T, nx)))


def penalty_of(P, value=0.3):
    """A finite penalty on every row but the last of each stage (that one stays hard)."""
    pen = np.full(P['d'].shape, float(value))
    pen[..., -1] = np.inf
    return pen


def variants(level):
    """The problems of shape (b) that an entry of this level is called with: [(name, problem)], every optional argument of the level in use in one of them."""
    b = shape_b()
    if level == 'hard':
        return [('rows', b)]
    if level == 'soft':
        return [('penalty', dict(b, penalty=penalty_of(b)))]
    rows, term = dict(b, **shape_b_rows()), dict(b, nt=-1)
    if level == 'eq':
        return [('rows', rows), ('terminal', term), ('rows-penalty', dict(rows, penalty=penalty_of(b, 5.0)))]
    return [('rows', dict(rows, aff=shape_b_affine(b, False))), ('terminal', dict(term, aff=shape_b_affine(b, True)))]


def reference_kwargs(P, b):
    """The keyword arguments of mpc_qp_affine_reference.closed_loop_aff for problem b (without x0, penalty, W)."""
    pick = lambda k: None if P[k] is None else P[k][b]
    kw = dict(q=pick('q'), Pf=P['Pf'][b], D=pick('D'), d=pick('d'), rows=None if P['ndcnt'] is None else P['ndcnt'][b], J=pick('J'), r=pick('r'), erows=pick('necnt'),
              Tx='constraint' if P['nt'] == -1 else pick('Tx'))
    if P['aff'] is not None:
        kw.update(offset=P['aff'][0][b], qf=P['aff'][1][b], trhs=None if P['aff'][2] is None else P['aff'][2][b])
    return kw


def out_shapes(P):
    nb, nx, mb, nd, N, ns, T, ne = (P[k] for k in ('nb', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'ne'))
    ntk = nx if P['nt'] < 0 else P['nt']
    f, i = np.float64, np.int32
    return dict(U0=((nb, ns, mb), f), XT=((nb, ns, nx), f), info=((nb, ns, 8), f), X=((nb, T + 1, ns, nx), f), U=((nb, T, ns, mb), f), iters=((nb, T, ns), i),
                nact=((nb, T, ns), i), hres=((nb, T, ns), f), Xol=((nb, ns, N + 1, nx), f), Uol=((nb, ns, N, mb), f), Lam=((nb, ns, N, nd), f),
                Eol=((nb, ns, N, nd), f), nviol=((nb, T, ns), i), Nu=((nb, ns, N, ne), f), NuT=((nb, ns, ntk), f), eres=((nb, T, ns), f))


def raw_call(lib, level, where, P, omit=(), refused=False, **over):
    """One call of the C entry of `level` on the host or the device.  Every output of the level is passed pre-filled (NaN, integers -7) unless named in `omit`
    (passed as NULL); over: arguments of P replaced for this call (sizes or arrays, e.g. a count out of range).  refused: the checks are expected to refuse
    the call, a device entry gets host addresses (it tests them for NULL and reads none), so that no device is needed.  Returns (rc, dict of the outputs as
    numpy arrays: what the entry left in the buffers)."""
    P = dict(P, **over)
    on_device = where == 'device' and not refused
    assert level != 'hard' or (P['penalty'] is None and not P['ne'] and not P['nt']), 'the hard entry has no such argument'
    assert level in ('eq', 'aff') or (not P['ne'] and not P['nt']), 'rows need the eq entry'
    assert level == 'aff' or P['aff'] is None, 'the affine arrays need the aff entry'
    names = REQUIRED + OPTIONAL + TAIL_OUT[level]
    outs = {k: np.full(sh, np.nan if dt is np.float64 else -7, dt) for k, (sh, dt) in out_shapes(P).items() if k in names and k not in omit}
    if on_device:
        import torch
        keep = {}

        def ptr(a, name=None):
            if a is None or not a.size:
                return None
            keep[name or len(keep)] = t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return C.c_void_p(t.data_ptr())
    else:
        def ptr(a, name=None):
            if a is None or not a.size:
                return None
            return a.ctypes.data_as(C.c_void_p if where == 'device' else C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))
    o = lambda k: ptr(outs.get(k), k)
    args = [P[k] for k in ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')] + [ptr(P[k]) for k in ('A', 'B', 'H', 'q', 'Pf', 'D', 'ndcnt', 'd', 'X0')] + [1e-10, 60]
    args += [o(k) for k in REQUIRED + OPTIONAL]
    if level != 'hard':
        args += [ptr(P['penalty']), o('Eol'), o('nviol')]
    if level in ('eq', 'aff'):
        args += [P['ne'], ptr(P['J']), ptr(P['r']), ptr(P['necnt']), P['nt'], ptr(P['Tx']), o('Nu'), o('NuT'), o('eres')]
    if level == 'aff':
        args += [ptr(a) for a in (P['aff'] or (None,) * 7)]
    if on_device:
        torch.cuda.synchronize()
    rc = getattr(lib, symbol(level, where))(*args)
    if on_device:
        torch.cuda.synchronize()
        outs = {k: (keep[k].cpu().numpy() if k in keep else v) for k, v in outs.items()}
    return rc, outs


def same_bits(a, b, keys):
    """The named outputs of two calls agree bit for bit (NaN included); -> the names that do not."""
    return [k for k in keys if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
