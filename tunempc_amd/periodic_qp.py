"""The periodic optimal-control QP on the GPU (csrc/tmpc_periodic_qp.h; include/tunempc_hip.h: tmpc_periodic_qp_batch_*): the orbit that the MPC layers of
tunempc_amd.mpc_qp take as their reference.  It is the LQ case of the reference's pocp.Pocp.solve (x_N = x_0 with x_0 free) and the QP subproblem of its
sqp_method.Sqp (stage costs and dynamics, stage inequality and equality rows, a periodicity constraint in place of an initial condition).  Per problem, with
N = periods p and k_j = j mod p,

    min   sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j),   z_j = [x_j; u_j],
    s.t.  x_{j+1} = A_k x_j + B_k u_j + c_k,  j = 0 .. N-1,  x_N := x_0  (x_0 is a variable),
          D_k z_j <= d_k (first ndcnt_k rows),   J_k z_j = r_k (first necnt_k rows).

q, c (offset), d, r make the answer non-zero; each is optional.  Rows are hard unless penalty= (c) or penalty2= (Z) is given; then row i of stage k is read
as the MPC step reads it (tunempc_amd.mpc_qp, the reference's slacked constraints sys['g'] / us of pocp.py):

    c = inf (Z = 0)  hard;    c > 0, Z = 0  D_i z - e <= d_i, e >= 0, cost c e (exact L1: the hard orbit while c exceeds the row's multiplier);
    c > 0, Z > 0     cost c e + 1/2 Z e^2;    c = 0, Z > 0  cost 1/2 Z e^2 (pure quadratic).
penalty2 without penalty: every row pure quadratic; penalty without penalty2: Z = 0.  A periodic problem whose bounds cannot all be met then returns the
least-penalised orbit instead of status 1 and NaN.  The weights are checked on the device, problem by problem: an invalid one (c negative or NaN, Z negative
or non-finite, Z != 0 on a hard row, c = 0 with Z = 0) gives that member status 3 and leaves the others alone.

Not served: warm starts (guess), a terminal cost (Pf has no meaning without an end): these keywords are refused with a ValueError.  Neither are the SQP
outer loop, nonlinear dynamics or the phase-fixing cost of pocp.py.

    periodic_qp_batch(A, B, H, ...)     the batch entry, numpy or torch (device tensors never leave the GPU)
    periodic_qp(A, B, Q, R, N, ...)     one model in the reference's calling style -> xref, uref as lists
    lds_bytes(nx, nu, nd, ne, soft)     the LDS layout of the header restated (soft: the layout of a call with penalty or penalty2)

Statuses are those of the MPC step: 0 Converged, 1 MaxIter, 2 NotConvex (also: no unique periodic trajectory, e.g. A = I, B = 0, c != 0), 3 NonFinite.  A
problem that does not converge returns NaN in its outputs; it never returns status 0.
"""
import numpy as np

from . import _lib
from . import lqr
from . import closed_loop as _cl
from . import mpc_qp as _mq
from .convexifier import _to_array

STATUS_NAMES = _mq.STATUS_NAMES
LDS_BYTES = _mq.LDS_BYTES
TOL, MAX_ITER = _mq.TOL, _mq.MAX_ITER
INFO_FIELDS = _mq.INFO_FIELDS
REFUSED_KEYWORDS = ('Pf', 'guess')


def lds_bytes(nx, nu, nd=0, ne=0, soft=False):
    """periodic_qp_lds of csrc/tmpc_periodic_qp.h restated: the bytes of LDS of a workgroup -- the hard / EQ layout of the MPC step (nt = 0), then M [nx x ldp],
    T [n x ldp], Gamma [nx x ldp], Gy [nu x ldp] and 10 vectors of ldp doubles, ldp = nx | 1.  soft: periodic_qp_soft_lds, the vectors e, nu, c, Z of the
    stage [nd] each after the hard layout (32 nd bytes more)."""
    nx, nu, nd, ne = int(nx), int(nu), int(nd), int(ne)
    ldp = nx | 1
    return _mq.lds_layout(nx, nu, nd, ne=ne)['bytes'] + 8 * ldp * (2 * nx + (nx + nu) + nu + 10) + (32 * nd if soft else 0)


def ws_doubles(nx, nu, nd, ne, N, soft=False):
    """periodic_qp_ws_doubles restated: doubles of workspace per slot.  soft: periodic_qp_soft_ws_doubles, E, NU, dE, C2 [N][nd] more."""
    return _mq.lds_layout(nx, nu, nd, ne=ne)['ws_doubles'](N) + N * nu * nx + N * nx + (4 * int(N) * int(nd) if soft else 0)


def _refuse(who, extra):
    bad = [k for k in REFUSED_KEYWORDS if k in extra]
    if bad:
        raise ValueError('{}: {} not served by the periodic QP (every start is cold, there is no terminal cost)'.format(who, ', '.join(bad)))
    if extra:
        raise TypeError('{}() got an unexpected keyword argument {!r}'.format(who, sorted(extra)[0]))


def _validate(who, A, B, H, q, offset, D, d, ndcnt, J, r, necnt, periods, tol, max_iter, penalty=None, penalty2=None):
    named = [('A', A), ('B', B), ('H', H)] + [(nm, x) for nm, x in (('q', q), ('offset', offset), ('D', D), ('d', d), ('J', J), ('r', r), ('penalty', penalty),
                                                                     ('penalty2', penalty2)) if x is not None]
    for nm, x in (('penalty', penalty), ('penalty2', penalty2)):
        if x is not None and not hasattr(x, 'shape'):
            raise ValueError('{}: {} must be an fp64 array [nb, p, nd] of the kind of A'.format(who, nm))
    use_torch = _cl._check_kind(who, named)
    if len(A.shape) != 4 or A.shape[2] != A.shape[3]:
        raise ValueError('{}: A [nb, p, nx, nx] expected, got {}'.format(who, tuple(A.shape)))
    nb, p, nx, _ = (int(v) for v in A.shape)
    if len(B.shape) != 4 or tuple(B.shape[:3]) != (nb, p, nx):
        raise ValueError('{}: B [nb, p, nx, nu] = [{}, {}, {}, nu] expected, got {}'.format(who, nb, p, nx, tuple(B.shape)))
    nu = int(B.shape[3])
    if nb < 1 or p < 1 or nx < 1 or nu < 1:
        raise ValueError('{}: nb, p, nx, nu >= 1 expected, got nb = {}, p = {}, nx = {}, nu = {}'.format(who, nb, p, nx, nu))
    n = nx + nu
    if tuple(H.shape) != (nb, p, n, n):
        raise ValueError('{}: H {} expected, got {}'.format(who, (nb, p, n, n), tuple(H.shape)))
    if isinstance(periods, bool) or not isinstance(periods, (int, np.integer)) or int(periods) < 1:
        raise ValueError('{}: periods must be an int >= 1, got {!r}'.format(who, periods))
    if q is not None and tuple(q.shape) != (nb, p, n):
        raise ValueError('{}: q {} expected, got {}'.format(who, (nb, p, n), tuple(q.shape)))
    if offset is not None and tuple(offset.shape) != (nb, p, nx):
        raise ValueError('{}: offset {} expected, got {}'.format(who, (nb, p, nx), tuple(offset.shape)))
    if (D is None) != (d is None):
        raise ValueError('{}: D and d come together (the rows D z <= d), got {} without {}'.format(who, *(('d', 'D') if D is None else ('D', 'd'))))
    if J is None and (r is not None or necnt is not None):
        raise ValueError('{}: {} describes the rows of J, which is None'.format(who, 'r' if r is not None else 'necnt'))
    if D is None and ndcnt is not None:
        raise ValueError('{}: ndcnt describes the rows of D, which is None'.format(who))
    for nm, x in (('penalty', penalty), ('penalty2', penalty2)):
        if D is None and x is not None:
            raise ValueError('{}: {} describes the rows of D, which is None'.format(who, nm))

    def counts(nm, cnt, cap):
        if not hasattr(cnt, 'shape') or lqr._is_torch(cnt) != use_torch:
            raise ValueError('{}: {} must be {} like A, B, H'.format(who, nm, 'a torch tensor' if use_torch else 'a numpy array'))
        if tuple(cnt.shape) != (nb, p) or 'int32' not in str(cnt.dtype):
            raise ValueError('{}: {} int32 {} expected, got {} {}'.format(who, nm, (nb, p), cnt.dtype, tuple(cnt.shape)))
        if use_torch and (not cnt.is_cuda or cnt.device != A.device):
            raise ValueError('{}: torch tensors must be tensors of one GPU ({}: {})'.format(who, nm, cnt.device))
        lo, hi = (int(cnt.min()), int(cnt.max()))
        if lo < 0 or hi > cap:
            raise ValueError('{}: {} in 0 .. {} expected, got {} .. {}'.format(who, nm, cap, lo, hi))
    nd = ne = 0
    if D is not None:
        if len(D.shape) != 4 or tuple(D.shape[:2]) != (nb, p) or int(D.shape[3]) != n or int(D.shape[2]) < 1:
            raise ValueError('{}: D [nb, p, nd, nx + nu] = [{}, {}, nd >= 1, {}] expected, got {}'.format(who, nb, p, n, tuple(D.shape)))
        nd = int(D.shape[2])
        if tuple(d.shape) != (nb, p, nd):
            raise ValueError('{}: d {} expected, got {}'.format(who, (nb, p, nd), tuple(d.shape)))
        if ndcnt is not None:
            counts('ndcnt', ndcnt, nd)
        for nm, x in (('penalty', penalty), ('penalty2', penalty2)):
            if x is not None and tuple(x.shape) != (nb, p, nd):
                raise ValueError('{}: {} {} expected, got {}'.format(who, nm, (nb, p, nd), tuple(x.shape)))
    if J is not None:
        if len(J.shape) != 4 or tuple(J.shape[:2]) != (nb, p) or int(J.shape[3]) != n or int(J.shape[2]) < 1:
            raise ValueError('{}: J [nb, p, ne, nx + nu] = [{}, {}, ne >= 1, {}] expected, got {}'.format(who, nb, p, n, tuple(J.shape)))
        ne = int(J.shape[2])
        if r is not None and tuple(r.shape) != (nb, p, ne):
            raise ValueError('{}: r {} expected, got {}'.format(who, (nb, p, ne), tuple(r.shape)))
        if necnt is not None:
            counts('necnt', necnt, ne)
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating)) or not float(tol) > 0.0:
        raise ValueError('{}: tol must be a float > 0, got {!r}'.format(who, tol))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError('{}: max_iter must be an int >= 1, got {!r}'.format(who, max_iter))
    if n > 64:
        raise NotImplementedError('{}: the periodic QP handles stage blocks up to nx + nu = 64 (got {})'.format(who, n))
    soft = penalty is not None or penalty2 is not None
    need = lds_bytes(nx, nu, nd, ne, soft)
    if need > LDS_BYTES:
        raise NotImplementedError('{}: nx = {}, nu = {} with room for {} {}rows and {} equality rows per stage needs {} bytes of LDS (limit {})'.format(
            who, nx, nu, nd, 'soft ' if soft else '', ne, need, LDS_BYTES))
    return use_torch


def periodic_qp_batch(A, B, H, q=None, offset=None, D=None, d=None, ndcnt=None, J=None, r=None, necnt=None, periods=1, tol=TOL, max_iter=MAX_ITER, penalty=None,
                      penalty2=None, **refused):
    """The periodic QP of the module docstring for nb problems in one launch.  A [nb,p,nx,nx], B [nb,p,nx,nu], H [nb,p,n,n] (used as (H + H') / 2); optional
    q [nb,p,n], offset c [nb,p,nx], D [nb,p,nd,n] with d [nb,p,nd] and ndcnt int32 [nb,p] (None: all nd rows), J [nb,p,ne,n] with r [nb,p,ne] (None: zero) and
    necnt int32 [nb,p]; periods: the horizon is N = periods p.  numpy arrays (staged through device buffers) or torch fp64 tensors of one GPU (the device entry:
    no host copy; the results are tensors of that GPU).  Returns a dict:
        X [nb,N,nx] (x_0 .. x_{N-1}), U [nb,N,nu], lam [nb,N,nd], nu [nb,N,ne],
        pi [nb,N,nx]: the multipliers of the dynamics, pi[:, 0] that of x_N = x_0, pi[:, j] that of x_j = A x_{j-1} + B u_{j-1} + c,
        cost [nb], status int32 [nb], iters int32 [nb], the info fields by name (status .. pivmin as float [nb]; steps is 1 on success),
        hres = max(D z - d) over all stages (-inf without rows), eres = max|J z - r|, per = max|A x_{N-1} + B u_{N-1} + c - x_0|   [nb] each.
    X[:, :p], U[:, :p] are what tunempc_amd.mpc_qp.about_reference takes as xref, uref (with periods = 1: X, U themselves).
    penalty, penalty2 [nb,p,nd] fp64 of the kind of A (module docstring: the row kinds; one of them may be None): with either the call goes through the soft
    entry and the dict gains eps [nb,N,nd] (the slack of every soft row, lam / Z on a pure quadratic row, 0 on hard and absent rows), nviol int32 [nb] (over
    all stages the two-pair rows with e > nu plus the pure rows with lam > s; -1 on a failed member), pcost [nb] (sum c e + 1/2 Z e^2; cost includes it) and
    emax [nb] (max e); hres stays max(D z - d), positive when a row is violated.  An invalid weight gives that member status 3.  Without them the call is
    the hard one, through the hard entry, and returns the keys above only.
    Pf and guess are refused with a ValueError (Not served, module docstring); shapes beyond the LDS layout (with a penalty: the soft layout) raise
    NotImplementedError before the library is touched."""
    who = 'periodic_qp_batch'
    _refuse(who, refused)
    use_torch = _validate(who, A, B, H, q, offset, D, d, ndcnt, J, r, necnt, periods, tol, max_iter, penalty, penalty2)
    cont = (lambda x: None if x is None else x.contiguous()) if use_torch else (lambda x: None if x is None else np.ascontiguousarray(x))
    soft = penalty is not None or penalty2 is not None
    if soft:
        args = [cont(x) for x in (A, B, H, q, offset, D, ndcnt, d, penalty, penalty2, J, r, necnt)]
        fn = _lib.periodic_qp_soft_batch_device if use_torch else _lib.periodic_qp_soft_batch_host
    else:
        args = [cont(x) for x in (A, B, H, q, offset, D, ndcnt, d, J, r, necnt)]
        fn = _lib.periodic_qp_batch_device if use_torch else _lib.periodic_qp_batch_host
    out = fn(*args, int(periods), float(tol), int(max_iter))
    info, res = out.pop('info'), out.pop('res')
    for i, nm in enumerate(INFO_FIELDS):
        out[nm] = info[:, i]
    if use_torch:
        import torch
        out['status'] = info[:, 0].to(torch.int32); out['iters'] = info[:, 2].to(torch.int32)
    else:
        out['status'] = info[:, 0].astype(np.int32); out['iters'] = info[:, 2].astype(np.int32)
    out.update(cost=res[:, 0], hres=res[:, 1], eres=res[:, 2], per=res[:, 3])
    if soft:
        out.update(pcost=res[:, 4], emax=res[:, 5])
    return out


def periodic_qp(A, B, Q, R, N, q=None, offset=None, D=None, d=None, J=None, r=None, periods=1, tol=TOL, max_iter=MAX_ITER, penalty=None, penalty2=None, **refused):
    """The periodic QP of one model in the reference's calling style: A, B, Q, R, N (the cross term) single matrices (p = 1) or lists of length p as in
    mpc_step; q, offset one vector or a list of p; D, d and J, r single arrays or ragged lists of p (None entries: no rows at that stage; r None: zero).
    Returns (xref, uref, info): xref, uref lists of periods p arrays (x_0 .. x_{N-1}, u_0 .. u_{N-1}), info a dict with X, U, lam, nu, pi, cost, status,
    iters, hres, eres, per and the info fields of periodic_qp_batch for this problem.  xref[:p], uref[:p] stacked are the xref, uref of
    tunempc_amd.mpc_qp.about_reference.  penalty, penalty2: the weights of the soft rows as mpc_step takes them -- one vector (every stage) or a ragged list
    of p vectors with one entry per row of D_k (None stages and np.inf entries are hard; penalty2 without penalty: the rows with Z > 0 are pure quadratic, the
    others hard) -- or one scalar for every row; info then gains eps, nviol, pcost, emax.  RuntimeError when the solve did not converge (no periodic
    trajectory, contradictory hard rows, not convex)."""
    who = 'periodic_qp'
    _refuse(who, refused)

    def rowwise(w):      # a scalar weight: that weight on every row of every stage
        if w is None or D is None or isinstance(w, (list, tuple)) or np.ndim(w) != 0:
            return w
        return [None if m is None else np.full(np.atleast_2d(_to_array(m)).shape[0], float(w)) for m in (D if isinstance(D, (list, tuple)) else [D] * len(A if isinstance(A, (list, tuple)) else [A]))]
    As, Bs, Hs, _, kw = _mq._stack_one(who, A, B, Q, R, N, np.zeros(np.atleast_2d(_to_array(A[0] if isinstance(A, (list, tuple)) else A)).shape[0]), D, d, q, None,
                                       rowwise(penalty), rowwise(penalty2))
    p, nx, nu = As.shape[1], As.shape[2], Bs.shape[3]
    eq = _mq._stack_eq(who, p, nx, nx + nu, J, r, None)
    cs = None
    if offset is not None:
        cl = [_to_array(v).astype(np.float64).reshape(-1) for v in (offset if isinstance(offset, (list, tuple)) else [offset] * p)]
        if len(cl) != p or any(v.shape != (nx,) for v in cl):
            raise ValueError('{}: offset must be one vector of nx = {} entries or a list of p = {} of them'.format(who, nx, p))
        cs = np.ascontiguousarray(np.stack(cl)[None])
    res = periodic_qp_batch(As, Bs, Hs, q=kw['q'], offset=cs, D=kw['D'], d=kw['d'], ndcnt=kw['ndcnt'], J=eq['J'], r=eq['r'], necnt=eq['necnt'], periods=periods,
                            tol=tol, max_iter=max_iter, **{k: kw[k] for k in ('penalty', 'penalty2') if kw.get(k) is not None})
    st = int(res['status'][0])
    if st != 0:
        raise RuntimeError('{}: the solve ended with status {} ({}) after {} iterations'.format(who, st, STATUS_NAMES.get(st), int(res['iters'][0])))
    info = {k: v[0] for k, v in res.items()}
    return [x.copy() for x in info['X']], [u.copy() for u in info['U']], info
