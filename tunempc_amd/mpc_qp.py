"""The inequality-constrained tracking-MPC step and its receding-horizon loop on the GPU: what the tracking MPC does when a deviation is large enough to hit
a bound (the reference's pmpc.py with h(x, u) >= 0 at every stage, as closed_loop_tools.check_equivalence and closed_loop_sim exercise it).

lqr.py and closed_loop.py serve the laws of a FIXED active set.  This module solves, per (problem, initial deviation x_0) and k_j = (phase0 + j) mod p,

    min  sum_{j<N} (1/2 z_j' H_k z_j + q_k' z_j) + 1/2 x_N' Pf_{k_N} x_N + qf_{k_N}' x_N,   z_j = [x_j; u_j],
    s.t. x_{j+1} = A_k x_j + B_k u_j + c_k,   D_k z_j <= d_k (first ndcnt_k rows of the stage),   j = 0 .. N-1,
         J_k z_j = r_k (first necnt_k rows of the stage),   Tx_{k_N} x_N = t_{k_N},  k_N = (phase0 + N) mod p   (J=, r=, necnt=, terminal=),
    (c, qf, t zero unless offset=, qf=, terminal_rhs= are given: the homogeneous problem in deviation coordinates),

where a row may be SOFT (`penalty`, the reference's preprocessing.add_mpc_slacks: D_i z - e_i <= d_i, e_i >= 0 at the cost c_i e_i, an exact L1 penalty: the
hard solution as long as c_i exceeds the row's multiplier, a violated row instead of an infeasible problem otherwise) or carry a QUADRATIC slack penalty
(`penalty2`: the cost c_i e_i + 1/2 Z_i e_i^2, or with c_i = 0 the pure quadratic 1/2 Z_i e_i^2, which keeps the control law smooth across the bound), the
equality rows are the reference's
g(x, u) = 0 and the terminal rows its p_operator(x_N - x_ref) = 0 in deviation coordinates (pmpc.py always carries one; terminal='constraint' is x_N = 0),

with a primal-dual interior-point method (Mehrotra's predictor-corrector, Riccati recursion with a Cholesky factorisation per stage), one 256-thread workgroup
per instance, the whole interior-point loop and all steps of the closed loop in one launch (csrc/tmpc_mpc_qp.h).

    mpc_qp_batch(A, B, H, X0, horizon, phase0=0, D=None, d=None, ...)              one step: u0, the open-loop X, U, lam
    mpc_closed_loop_batch(A, B, H, X0, horizon, steps, phase0=0, ...)              the receding-horizon loop on the linear plant
    mpc_step(A, B, Q, R, N, x0, horizon, ...)                                      one model in the reference's calling style
    mpc_closed_loop_sim(A, B, Q, R, N, x0, horizon, steps, ...)                    -> the reference's log {'x', 'u', 'l', 'h'} (and 'usc' with penalty=)
    slack_penalty(lam_h, active_set, slack_flag, factor)                           the reference's rule for the weights of the soft rows
    about_reference(A, B, H, xref, uref, ...)                                      a deviation problem and a periodic reference -> the absolute-coordinate kwargs
    mpc_qp_gain_batch(A, B, H, sol, horizon, phase0=0, ...)                        the law at a solved step: K0 = -du0/dx0 at the active set of sol, strict
    mpc_step_gain(A, B, Q, R, N, sol, horizon, ...)                                one model in the reference's calling style, beside mpc_step
    mpc_gain_equivalence_batch(A, B, H, Hc, X0, horizon, P=None, ...)              the certificate: both QPs solved, the gains of H and Hc at one active set

The affine problem (offset=, qf=, terminal_rhs=; in the loop plant=, disturbance=) is the reference's controller in ABSOLUTE coordinates -- its cost
(w - wref)' H (w - wref) + q' w, its terminal row p_operator(x_N - x_ref) = 0, x0 the plant state --, the model x+ = A x + B u + c of a linearisation that is
not taken on a trajectory of the model or of an estimated constant disturbance, and the loop on a plant that is not the prediction model:
x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t.  It runs on AFF instantiations of the two kernels that serve J= and terminal= (with no rows at all when there
are none); without any of the five arguments every call is the one it was.

An equality row is a hard row without a slack: a multiplier of free sign at the constant barrier weight 1e12 (csrc/tmpc_mpc_qp.h states the rules).  An
instance whose rows cannot be met -- horizon * nu too short to reach Tx x_N = 0, a row of stage 0 on x_0 alone that x_0 violates (the reference drops state-only
h rows at stage 0 for the same reason) -- is infeasible and ends with status 1, like contradictory inequality rows.

Warm starts (guess=, guess_shift=, warm=, warm_floor=; csrc/tmpc_mpc_qp.h states the rule, the WARM instantiations run it): a step may start from the solution
of an earlier call (guess=, shifted by one stage with guess_shift=1 when it comes from the previous phase), and the steps t > 0 of a loop from the shifted
iterate of step t - 1 (warm=True), as the reference's Pmpc.step always does.  mpc_closed_loop_plant runs the loop against any plant callback, one launch per
step: the reference's closed_loop_sim(F=...) on a plant that is not linear.

Not served: more than nx terminal rows; the nonlinear plant inside one launch (mpc_closed_loop_plant steps it from Python).  Conventions as in lqr.py / closed_loop.py.  There is no CPU path: the solve runs in the HIP library or the call raises."""
import functools
import inspect

import numpy as np

from . import _lib
from . import lqr
from . import closed_loop as _cl
from .convexifier import _to_array

STATUS_NAMES = {0: 'Converged', 1: 'MaxIter', 2: 'NotConvex', 3: 'NonFinite'}
LDS_BYTES = 160 * 1024
TOL = 1e-10            # the defaults of tests/mpc_qp_reference.py
MAX_ITER = 60
SLOTS = 512            # workgroups (workspace slots) of a launch at the most
INFO_FIELDS = ('status', 'steps', 'iters_total', 'iters_max', 'mu', 'rp', 'rd', 'pivmin')


def lds_layout(nx, nu, nd=0, soft=False, ne=None, nt=0, quad=False):
    """mpc_qp_lds of csrc/tmpc_mpc_qp.h restated: dict bytes (LDS of a workgroup), ws_doubles (function of the horizon: doubles of workspace per slot).
    soft: mpc_qp_soft_lds / mpc_qp_soft_ws_doubles, the layout of a call with penalty (the vectors e, nu, c after the hard layout, E, NU, dE, C2 after the hard
    workspace).  ne (not None): mpc_qp_eq_lds / mpc_qp_eq_ws_doubles, the layout of a call with J= or terminal= (J_k [ne x ld] and three vectors after the hard
    or soft layout, NUe, REQ [N][ne] and NUT [nt] after the workspace).  quad: mpc_qp_quad_layout, the layout of a call with penalty2 (the vector Z [nd] after the
    soft layout, the soft workspace; with ne after that layout)."""
    nx, nu, nd = int(nx), int(nu), int(nd)
    n = nx + nu
    ld, ldp, lv = (n + 1) | 1, nx | 1, max(n + 1, nd)
    total = nx * ld + nx * ldp + nx * ld + n * ld + nd * ld + 24 * lv + 8
    if ne is not None:
        ne, nt = int(ne), int(nt)
        base = lds_layout(nx, nu, nd, soft, quad=quad)
        return dict(bytes=base['bytes'] + 8 * ne * (ld + 3), ws_doubles=lambda N: base['ws_doubles'](N) + 2 * N * ne + nt)
    if quad:
        base = lds_layout(nx, nu, nd, soft=True)
        return dict(bytes=base['bytes'] + 8 * nd, ws_doubles=base['ws_doubles'])
    if soft:
        return dict(bytes=8 * (total + 3 * nd), ws_doubles=lambda N: 2 * (N + 1) * n + 6 * N * nd + N * nx + N * nu * (n + 1) + 4 * N * nd)
    return dict(bytes=8 * total, ws_doubles=lambda N: 2 * (N + 1) * n + 6 * N * nd + N * nx + N * nu * (n + 1))


WARM_FLOOR = 1e-2      # delta of the warm start's floors (absolute; tests/mpc_qp_warm_reference.py and profiles/mpc_qp_warm_reference_counts.txt)
HIDDEN_KEYWORDS = ('penalty2', 'guess', 'guess_shift', 'warm', 'warm_floor')
WARM_KEYWORDS = HIDDEN_KEYWORDS[1:]


def _hidden_keywords(f):
    """The parameters of f named in HIDDEN_KEYWORDS (penalty2 and the warm-start keywords) are the last of the four calls and keyword-only: they are taken off
    the call here and handed to f by name.  The signature that introspection reports stays the parameter list the call had before they existed -- everything up
    to terminal, which callers and tools pin to tell that a positional call keeps its meaning --; the docstring names them.  warm_call (the last parameter of
    f, hidden too, not for callers) tells f whether any of WARM_KEYWORDS was PASSED, whatever its value: such a call goes through the warm entry and returns
    `warm`, also with warm=False or warm_floor=1e-2 spelled out."""
    sig = inspect.signature(f)
    hidden = [p for p in sig.parameters.values() if p.name in HIDDEN_KEYWORDS]

    @functools.wraps(f)
    def call(*args, **kw):
        return f(*args, **{**{p.name: p.default for p in hidden}, 'warm_call': any(k in kw for k in WARM_KEYWORDS), **kw})
    del call.__wrapped__
    call.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.name not in HIDDEN_KEYWORDS + ('warm_call',)])
    return call


GUESS_KEYS = ('X', 'U', 'lam', 'eps', 'nu', 'nu_term')


def _validate_warm(who, use_torch, A, B, X0, N, nd, penalty, penalty2, J, terminal, guess, guess_shift, warm, warm_floor, force=False):
    """The warm-start keywords, after _validate -> None when none of them is used (the call is routed where it was), else the tuple (flags, floor, Xg, Ug, Lamg,
    Eg, Nug, NuTg) of the warm entries.  guess: a dict as returned by an earlier mpc_qp_batch: X, U, lam (with rows) and eps (with penalty or penalty2), nu
    (with J), nu_term (with terminal), of the shapes that call returns.  force: the warm entry also without any of them (mpc_closed_loop_plant: every step of
    its loop returns the same keys)."""
    if not force and guess is None and warm is False and guess_shift == 0 and warm_floor == WARM_FLOOR:
        return None
    if isinstance(warm, (bool, np.bool_)) is False:
        raise ValueError('{}: warm must be a bool, got {!r}'.format(who, warm))
    if isinstance(guess_shift, bool) or guess_shift not in (0, 1):
        raise ValueError('{}: guess_shift must be 0 (a guess for the same phase) or 1 (a guess from the previous phase), got {!r}'.format(who, guess_shift))
    if guess_shift and guess is None:
        raise ValueError('{}: guess_shift describes guess, which is None'.format(who))
    if isinstance(warm_floor, bool) or not isinstance(warm_floor, (int, float, np.floating)) or not 0.0 < float(warm_floor) < float('inf'):
        raise ValueError('{}: warm_floor must be a finite float > 0, got {!r}'.format(who, warm_floor))
    arrays = (None,) * 6
    if guess is not None:
        if not isinstance(guess, dict):
            raise ValueError('{}: guess must be a dict as returned by mpc_qp_batch (X, U, lam, and eps, nu, nu_term where the problem has them), got {}'.format(
                who, type(guess).__name__))
        nb, ns, nx, nu = int(X0.shape[0]), int(X0.shape[1]), int(X0.shape[2]), int(B.shape[3])
        ne = 0 if J is None else int(J.shape[2])
        nt = 0 if terminal is None else (nx if isinstance(terminal, str) else int(terminal.shape[2]))
        want = [('X', (nb, ns, N + 1, nx), True), ('U', (nb, ns, N, nu), True), ('lam', (nb, ns, N, nd), nd > 0),
                ('eps', (nb, ns, N, nd), nd > 0 and (penalty is not None or penalty2 is not None)), ('nu', (nb, ns, N, ne), ne > 0), ('nu_term', (nb, ns, nt), nt > 0)]
        got = []
        for key, shape, needed in want:
            x = guess.get(key)
            if not needed:
                got.append(None)
                continue
            if x is None:
                raise ValueError('{}: guess[{!r}] {} expected, got None (a call with return_traj=False returns no guess)'.format(who, key, shape))
            if not hasattr(x, 'shape') or tuple(x.shape) != shape:
                raise ValueError('{}: guess[{!r}] {} expected, got {}'.format(who, key, shape, tuple(x.shape) if hasattr(x, 'shape') else type(x).__name__))
            got.append(x)
        _cl._check_kind(who, [('A', A)] + [('guess[%r]' % k, x) for (k, _, _), x in zip(want, got) if x is not None])
        arrays = tuple(None if x is None else lqr._contig(x, use_torch) for x in got)
    flags = (1 if warm else 0) | (2 if guess is not None else 0) | (4 if guess is not None and guess_shift else 0)
    return (flags, float(warm_floor)) + arrays


def _check_penalty2(who, penalty, penalty2):
    """The values of penalty beside penalty2 (arrays of one shape, numpy or torch): Z finite and >= 0, 0 on a hard row; c > 0, or 0 beside a Z > 0."""
    inf = float('inf')
    if not bool(((penalty2 >= 0) & (penalty2 < inf)).all()):                # (NaN fails the comparisons)
        raise ValueError('{}: penalty2 finite and >= 0 expected in every entry, got min {}, max {}'.format(who, float(penalty2.min()), float(penalty2.max())))
    if bool(((penalty == inf) & (penalty2 != 0)).any()):
        raise ValueError('{}: penalty2 = 0 expected on every hard row (penalty = inf)'.format(who))
    if not bool(((penalty > 0) | ((penalty == 0) & (penalty2 > 0))).all()):
        raise ValueError('{}: penalty > 0 expected in every entry (inf: a hard row), or 0 beside a penalty2 > 0 (a pure quadratic row), got min {}'.format(
            who, float(penalty.min())))


def _validate(who, A, B, H, X0, horizon, phase0, D, d, ndcnt, q, Pf, tol, max_iter, steps=1, penalty=None, J=None, r=None, necnt=None, terminal=None,
              penalty2=None):
    if terminal is not None and not (isinstance(terminal, str) and terminal == 'constraint') and not hasattr(terminal, 'shape'):
        raise ValueError("{}: terminal must be None, 'constraint' or an array [nb, p, nt, nx], got {!r}".format(who, terminal))
    Tx = terminal if hasattr(terminal, 'shape') else None
    named = [('A', A), ('B', B), ('H', H), ('X0', X0)] + [(nm, x) for nm, x in (('D', D), ('d', d), ('q', q), ('Pf', Pf), ('penalty', penalty), ('J', J), ('r', r),
                                                                                 ('terminal', Tx), ('penalty2', penalty2)) if x is not None]
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
    if len(X0.shape) != 3 or int(X0.shape[0]) != nb or int(X0.shape[2]) != nx:
        raise ValueError('{}: X0 [nb, ns, nx] = [{}, ns, {}] expected, got {}'.format(who, nb, nx, tuple(X0.shape)))
    ns = int(X0.shape[1])
    if ns < 1:
        raise ValueError('{}: ns >= 1 initial states expected, got X0 {}'.format(who, tuple(X0.shape)))
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or int(horizon) < 1:
        raise ValueError('{}: horizon must be an int >= 1, got {!r}'.format(who, horizon))
    T, k0 = _cl._validate_steps(who, steps, phase0, p)
    if (D is None) != (d is None):
        raise ValueError('{}: D and d come together (the rows D z <= d), got {} without {}'.format(who, *(('d', 'D') if D is None else ('D', 'd'))))
    if D is None and ndcnt is not None:
        raise ValueError('{}: ndcnt describes the rows of D, which is None'.format(who))
    if D is None and penalty2 is not None:
        raise ValueError('{}: penalty2 describes the rows of D, which is None'.format(who))
    if D is None and penalty is not None:
        raise ValueError('{}: penalty describes the rows of D, which is None'.format(who))
    nd = 0
    if D is not None:
        if len(D.shape) != 4 or tuple(D.shape[:2]) != (nb, p) or int(D.shape[3]) != n or int(D.shape[2]) < 1:
            raise ValueError('{}: D [nb, p, nd, nx + nu] = [{}, {}, nd >= 1, {}] expected, got {}'.format(who, nb, p, n, tuple(D.shape)))
        nd = int(D.shape[2])
        if tuple(d.shape) != (nb, p, nd):
            raise ValueError('{}: d {} expected, got {}'.format(who, (nb, p, nd), tuple(d.shape)))
        if ndcnt is not None:
            if not hasattr(ndcnt, 'shape') or lqr._is_torch(ndcnt) != use_torch:
                raise ValueError('{}: ndcnt must be {} like A, B, H'.format(who, 'a torch tensor' if use_torch else 'a numpy array'))
            if tuple(ndcnt.shape) != (nb, p) or 'int32' not in str(ndcnt.dtype):
                raise ValueError('{}: ndcnt int32 {} expected, got {} {}'.format(who, (nb, p), ndcnt.dtype, tuple(ndcnt.shape)))
            if use_torch and (not ndcnt.is_cuda or ndcnt.device != A.device):
                raise ValueError('{}: torch tensors must be tensors of one GPU (ndcnt: {})'.format(who, ndcnt.device))
            lo, hi = (int(ndcnt.min()), int(ndcnt.max()))
            if lo < 0 or hi > nd:
                raise ValueError('{}: ndcnt in 0 .. nd = {} expected, got {} .. {}'.format(who, nd, lo, hi))
    if q is not None and tuple(q.shape) != (nb, p, n):
        raise ValueError('{}: q {} expected, got {}'.format(who, (nb, p, n), tuple(q.shape)))
    if Pf is not None and tuple(Pf.shape) != (nb, p, nx, nx):
        raise ValueError('{}: Pf {} expected, got {}'.format(who, (nb, p, nx, nx), tuple(Pf.shape)))
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating)) or not float(tol) > 0.0:
        raise ValueError('{}: tol must be a float > 0, got {!r}'.format(who, tol))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 1:
        raise ValueError('{}: max_iter must be an int >= 1, got {!r}'.format(who, max_iter))
    if n > 64:
        raise NotImplementedError('{}: the MPC step handles stage blocks up to nx + nu = 64 (got {})'.format(who, n))
    lay = lds_layout(nx, nu, nd)
    if lay['bytes'] > LDS_BYTES:
        raise NotImplementedError('{}: nx = {}, nu = {} with room for {} rows per stage needs {} bytes of LDS (limit {})'.format(who, nx, nu, nd, lay['bytes'], LDS_BYTES))
    if penalty is not None:
        if tuple(penalty.shape) != (nb, p, nd):
            raise ValueError('{}: penalty {} expected, got {}'.format(who, (nb, p, nd), tuple(penalty.shape)))
        if penalty2 is None and not bool((penalty > 0).all()):              # (NaN fails the comparison)
            raise ValueError('{}: penalty > 0 expected in every entry (inf: a hard row), got min {}'.format(who, float(penalty.min())))
        soft = lds_layout(nx, nu, nd, soft=True)
        if soft['bytes'] > LDS_BYTES:
            raise NotImplementedError('{}: nx = {}, nu = {} with room for {} soft rows per stage needs {} bytes of LDS (limit {})'.format(
                who, nx, nu, nd, soft['bytes'], LDS_BYTES))
    if penalty2 is not None:                                                # (after _run: penalty is an array, zeros where the caller gave None)
        if tuple(penalty2.shape) != (nb, p, nd):
            raise ValueError('{}: penalty2 {} expected, got {}'.format(who, (nb, p, nd), tuple(penalty2.shape)))
        _check_penalty2(who, penalty, penalty2)
        quad = lds_layout(nx, nu, nd, quad=True)
        if quad['bytes'] > LDS_BYTES:
            raise NotImplementedError('{}: nx = {}, nu = {} with room for {} rows with quadratic penalties per stage needs {} bytes of LDS (limit {})'.format(
                who, nx, nu, nd, quad['bytes'], LDS_BYTES))
    if J is None and (r is not None or necnt is not None):
        raise ValueError('{}: {} describes the rows of J, which is None'.format(who, 'r' if r is not None else 'necnt'))
    ne = 0
    if J is not None:
        if len(J.shape) != 4 or tuple(J.shape[:2]) != (nb, p) or int(J.shape[3]) != n or int(J.shape[2]) < 1:
            raise ValueError('{}: J [nb, p, ne, nx + nu] = [{}, {}, ne >= 1, {}] expected, got {}'.format(who, nb, p, n, tuple(J.shape)))
        ne = int(J.shape[2])
        if r is not None and tuple(r.shape) != (nb, p, ne):
            raise ValueError('{}: r {} expected, got {}'.format(who, (nb, p, ne), tuple(r.shape)))
        if necnt is not None:
            if not hasattr(necnt, 'shape') or lqr._is_torch(necnt) != use_torch:
                raise ValueError('{}: necnt must be {} like A, B, H'.format(who, 'a torch tensor' if use_torch else 'a numpy array'))
            if tuple(necnt.shape) != (nb, p) or 'int32' not in str(necnt.dtype):
                raise ValueError('{}: necnt int32 {} expected, got {} {}'.format(who, (nb, p), necnt.dtype, tuple(necnt.shape)))
            if use_torch and (not necnt.is_cuda or necnt.device != A.device):
                raise ValueError('{}: torch tensors must be tensors of one GPU (necnt: {})'.format(who, necnt.device))
            lo, hi = (int(necnt.min()), int(necnt.max()))
            if lo < 0 or hi > ne:
                raise ValueError('{}: necnt in 0 .. ne = {} expected, got {} .. {}'.format(who, ne, lo, hi))
    nt = 0 if terminal is None else nx
    if Tx is not None:
        if len(Tx.shape) != 4 or tuple(Tx.shape[:2]) != (nb, p) or int(Tx.shape[3]) != nx or not 1 <= int(Tx.shape[2]) <= nx:
            raise ValueError('{}: terminal [nb, p, nt, nx] = [{}, {}, 1 <= nt <= {}, {}] expected, got {}'.format(who, nb, p, nx, nx, tuple(Tx.shape)))
        nt = int(Tx.shape[2])
    if J is not None or terminal is not None:
        lay = lds_layout(nx, nu, nd, soft=penalty is not None, ne=ne, nt=nt, quad=penalty2 is not None)
        if lay['bytes'] > LDS_BYTES:
            raise NotImplementedError('{}: nx = {}, nu = {} with room for {} {}rows and {} equality rows per stage needs {} bytes of LDS (limit {})'.format(
                who, nx, nu, nd, 'soft ' if penalty is not None else '', ne, lay['bytes'], LDS_BYTES))
    return use_torch, nd, int(horizon), T, k0


def _validate_affine(who, use_torch, A, B, X0, T, terminal, offset, qf, terminal_rhs, plant, disturbance):
    """The arguments of the affine problem, after _validate -> (offset, qf, terminal_rhs, Ap, Bp, cp, W), None or an array each."""
    nb, p, nx, _ = (int(v) for v in A.shape)
    nu, ns = int(B.shape[3]), int(X0.shape[1])
    if plant is not None:
        if not isinstance(plant, (tuple, list)) or len(plant) not in (2, 3):
            raise ValueError('{}: plant must be (Ap, Bp) or (Ap, Bp, cp), got {!r}'.format(who, type(plant).__name__ if not isinstance(plant, (tuple, list)) else len(plant)))
        if plant[0] is None or plant[1] is None:
            raise ValueError('{}: plant (Ap, Bp[, cp]): Ap and Bp come together, neither may be None'.format(who))
    Ap, Bp, cp = (tuple(plant) + (None,))[:3] if plant is not None else (None, None, None)
    named = [(nm, x) for nm, x in (('offset', offset), ('qf', qf), ('terminal_rhs', terminal_rhs), ('plant[0]', Ap), ('plant[1]', Bp), ('plant[2]', cp),
                                   ('disturbance', disturbance)) if x is not None]
    if not named:
        return None
    _cl._check_kind(who, [('A', A)] + named)
    if terminal_rhs is not None and terminal is None:
        raise ValueError('{}: terminal_rhs describes the rows of terminal, which is None'.format(who))
    nt = 0 if terminal is None else (nx if isinstance(terminal, str) else int(terminal.shape[2]))
    for nm, x, shape in (('offset', offset, (nb, p, nx)), ('qf', qf, (nb, p, nx)), ('terminal_rhs', terminal_rhs, (nb, p, nt)), ('plant[0]', Ap, (nb, p, nx, nx)),
                         ('plant[1]', Bp, (nb, p, nx, nu)), ('plant[2]', cp, (nb, p, nx)), ('disturbance', disturbance, (nb, ns, T, nx))):
        if x is not None and tuple(x.shape) != shape:
            raise ValueError('{}: {} {} expected, got {}'.format(who, nm, shape, tuple(x.shape)))
    return tuple(lqr._contig(x, use_torch) for x in (offset, qf, terminal_rhs, Ap, Bp, cp, disturbance))


def _run(who, A, B, H, X0, horizon, steps, phase0, D, d, ndcnt, q, Pf, tol, max_iter, return_traj, return_ol, penalty=None, J=None, r=None, necnt=None,
         terminal=None, offset=None, qf=None, terminal_rhs=None, plant=None, disturbance=None, penalty2=None, guess=None, guess_shift=0, warm=False,
         warm_floor=WARM_FLOOR, force_warm=False):
    if penalty2 is not None and penalty is None and hasattr(penalty2, 'shape'):      # every row pure quadratic: penalty is taken as 0
        penalty = penalty2.new_zeros(tuple(penalty2.shape)) if lqr._is_torch(penalty2) else np.zeros(penalty2.shape)
    use_torch, nd, N, T, k0 = _validate(who, A, B, H, X0, horizon, phase0, D, d, ndcnt, q, Pf, tol, max_iter, steps, penalty, J, r, necnt, terminal, penalty2)
    aff = _validate_affine(who, use_torch, A, B, X0, T, terminal, offset, qf, terminal_rhs, plant, disturbance)
    wm = _validate_warm(who, use_torch, A, B, X0, N, nd, penalty, penalty2, J, terminal, guess, guess_shift, warm, warm_floor, force_warm)
    if aff is not None and J is None and terminal is None:                  # the AFF kernels are EQ kernels: their layout with no rows
        lay = lds_layout(A.shape[2], B.shape[3], nd, soft=penalty is not None, ne=0, nt=0, quad=penalty2 is not None)
        if lay['bytes'] > LDS_BYTES:
            raise NotImplementedError('{}: nx = {}, nu = {} with room for {} rows per stage needs {} bytes of LDS (limit {})'.format(
                who, A.shape[2], B.shape[3], nd, lay['bytes'], LDS_BYTES))
    A, B, H, X0, D, d, q, Pf, penalty, J, r = (lqr._contig(x, use_torch) for x in (A, B, H, X0, D, d, q, Pf, penalty, J, r))
    if ndcnt is not None:
        ndcnt = ndcnt.contiguous() if use_torch else np.ascontiguousarray(ndcnt)
    if necnt is not None:
        necnt = necnt.contiguous() if use_torch else np.ascontiguousarray(necnt)
    # the entry of the lowest level that has the arguments: hard, soft (penalty), eq (J, terminal), aff (the affine arrays); each level appends its own
    level = 'aff_' if aff is not None else 'eq_' if J is not None or terminal is not None else 'soft_' if penalty is not None else ''
    args = (A, B, H, q, Pf, D, ndcnt, d) + ((penalty,) if level else ())
    if level in ('eq_', 'aff_'):
        args += (J, r, necnt, terminal if isinstance(terminal, str) or terminal is None else lqr._contig(terminal, use_torch)) + ((aff,) if level == 'aff_' else ())
    if penalty2 is not None:                                                # the quad entry: the arguments of the aff entry (aff None: no affine array), then penalty2
        level = 'quad_'
        args = (A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, terminal if isinstance(terminal, str) or terminal is None else lqr._contig(terminal, use_torch),
                aff, lqr._contig(penalty2, use_torch))
    if wm is not None:                                                      # the warm entry: the arguments of the quad entry (penalty, aff, penalty2 None where there is none), then wm
        level = 'warm_'
        args = (A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, terminal if isinstance(terminal, str) or terminal is None else lqr._contig(terminal, use_torch),
                aff, None if penalty2 is None else lqr._contig(penalty2, use_torch), wm)
    entry = getattr(_lib, 'mpc_qp_%sbatch_%s' % (level, 'device' if use_torch else 'host'))
    out = entry(*args, X0, N, T, k0, float(tol), int(max_iter), bool(return_traj), bool(return_ol))
    info = out['info']
    for i, name in enumerate(INFO_FIELDS):
        col = info[..., i]
        if i < 4:
            col = col.to(__import__('torch').int32) if use_torch else col.astype(np.int32)
        else:
            col = col.clone() if use_torch else col.copy()
        out[name] = col
    return out


@_hidden_keywords
def mpc_qp_batch(A, B, H, X0, horizon, phase0=0, D=None, d=None, ndcnt=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER, return_traj=True, offset=None,
                 qf=None, terminal_rhs=None, penalty=None, J=None, r=None, necnt=None, terminal=None, penalty2=None, guess=None, guess_shift=0,
                 warm_floor=WARM_FLOOR, warm_call=False):
    """One MPC step per (problem, initial deviation): A [nb,p,nx,nx], B [nb,p,nx,nu], H [nb,p,n,n] (used as (H + H') / 2), X0 [nb,ns,nx], fp64, n = nx + nu <= 64;
    the horizon-`horizon` QP from phase `phase0`.  Optional: the rows D [nb,p,nd,n], d [nb,p,nd] (D z <= d; ndcnt int32 [nb,p]: only the first ndcnt rows of a
    stage, None: all nd), q [nb,p,n] (linear cost), Pf [nb,p,nx,nx] (terminal weight 1/2 x_N' Pf[(phase0 + N) mod p] x_N); None: absent / zero.  Without rows
    this is the plain horizon-N LQ problem.  tol, max_iter: the stop rule of csrc/tmpc_mpc_qp.h (residuals and mu relative to the scale of the problem).
    penalty [nb,p,nd] (fp64): inf a hard row, c > 0 a soft row (D_i z - e_i <= d_i, e_i >= 0, cost c e_i at every stage); None: every row hard, the call as it
    was.  With a penalty the dict gains eps [nb,ns,N,nd] (the open-loop slacks; 0 on hard rows; None with return_traj=False) and nviol [nb,ns] int32 (rows of
    stage 0 with e > nu), hres > 0 tells a violated soft row, and a state outside a soft bound is no longer status 1.
    J [nb,p,ne,n], r [nb,p,ne] (None: zero), necnt int32 [nb,p] (None: all ne): the equality rows J_k z_j = r_k of every stage.  terminal: 'constraint' (x_N = 0)
    or Tx [nb,p,nt,nx], 1 <= nt <= nx, indexed by (phase0 + N) mod p like Pf: the rows Tx x_N = 0.  With J or terminal the dict gains nu [nb,ns,N,ne] and
    nu_term [nb,ns,nt] (the multipliers, free sign; None with return_traj=False) and eres [nb,ns] = max|J z_0 - r| (0 at a stage without rows).  Rows that
    cannot be met (horizon * nu too short to reach the terminal rows, a row of stage 0 on x_0 alone that x_0 violates) make the instance infeasible: status 1.
    Without them (J=None, terminal=None) the call is the one it was, bit for bit.
    offset [nb,p,nx]: the dynamics are x_{j+1} = A_k x_j + B_k u_j + offset_k (indexed by the phase like A); qf [nb,p,nx]: the terminal cost gains
    qf[(phase0 + N) mod p]' x_N (legal without Pf); terminal_rhs [nb,p,nt] ([nb,p,nx] with terminal='constraint': x_N = t): the terminal rows read
    Tx x_N = terminal_rhs[(phase0 + N) mod p]; it needs terminal=.  With any of the three the dict also holds nu, nu_term (empty without rows) and eres, x1
    is A x_0 + B u_0 + offset, a non-finite entry that the step meets makes the instance status 3 and a terminal_rhs that cannot be reached status 1.
    Without them the call is the one it was, bit for bit.
    penalty2 [nb,p,nd] (fp64, the last keyword, to be passed by keyword only; inspect.signature lists the parameters up to terminal): the L2 weight Z >= 0 of every row beside its L1 weight c = penalty.  c = inf: a hard row (Z must be 0);
    c > 0, Z = 0: the soft row above, with its bits; c > 0, Z > 0: the cost c e + 1/2 Z e^2 (exact while c exceeds the multiplier, large violations still
    punished); c = 0, Z > 0: the pure quadratic 1/2 Z e^2 (e = lam / Z; the control law stays smooth across the bound; no multiplier estimate is needed to choose
    a weight).  penalty2 with penalty=None: every row pure quadratic.  eps holds the slack of every soft row (lam / Z on a pure row), nviol counts the
    two-pair rows with e > nu and the pure rows with lam > s (on a pure row active means violated).  The dict also holds nu, nu_term (empty without rows) and
    eres.  Without penalty2 the call is routed exactly where it was.  about_reference builds the three from a periodic reference.  In the signatures of the four calls the
    three (and plant, disturbance) stand between return_traj / max_iter and penalty: what comes before them is where it was, and penalty, J, r, necnt, terminal
    stay the last parameters, so every argument from penalty on is to be passed by keyword.
    guess, guess_shift=0, warm_floor=1e-2 (keyword-only like penalty2, not listed by inspect.signature): the warm start.  guess is a dict as returned by an
    earlier mpc_qp_batch of the same shapes -- X, U, lam, and eps, nu, nu_term where the problem has them (ValueError when one of those is None or has the wrong
    shape) --; guess_shift=0: a guess for the same phase (a neighbouring x_0), everything as given and x_0 replaced; guess_shift=1: a guess from the previous
    phase, shifted by one stage (stage j takes stage j + 1, u_{N-1} repeats, x_N = A x_{N-1} + B u_{N-1} + offset, the new last stage's multipliers zero,
    nu_term kept).  Slacks and multipliers are floored at warm_floor by row kind (csrc/tmpc_mpc_qp.h).  An instance whose guess holds a non-finite entry (a
    failed predecessor returns NaN) starts cold; a warm-started solve that ends with status 1 or 2 is solved again from the cold start and the iteration
    counts add up -- an infeasible instance costs two runs of max_iter, and iters_total / iters_max (which may then exceed max_iter) and pivmin cover both
    attempts --; status 3 is not retried.  A call that PASSES any of these keywords, whatever the value, returns `warm` [nb,ns]
    int32 in addition (0 cold, 1 the warm start delivered, 2 the cold restart delivered, -1 failed) and nu, nu_term (empty without rows), eres.  Without them
    the call is routed exactly where it was.

    numpy arrays run through the host entry; torch tensors on a GPU through the device entry (torch tensors out, the inputs are not copied).  Both run the same
    kernel and agree bit for bit; the numbers of an instance do not depend on ns or on the other instances of the call.

    Returns dict: u0 [nb,ns,nu], X [nb,ns,N+1,nx], U [nb,ns,N,nu], lam [nb,ns,N,nd] (the open-loop solution; None with return_traj=False), nact [nb,ns] int32
    (rows of stage 0 with lam > s), hres [nb,ns] = max(D z_0 - d) (-inf at a stage without rows), x1 [nb,ns,nx] = A x_0 + B u_0, and the info fields status
    (0 converged, 1 max_iter reached -- an infeasible instance ends here --, 2 a stage matrix not positive definite: not convex along the path, 3 non-finite), steps,
    iters_total, iters_max [nb,ns] int32, mu, rp, rd, pivmin [nb,ns], info [nb,ns,8].  An instance with status != 0 returns NaN (nact -1); the others are not
    affected.  ValueError: shapes, dtypes, mixed numpy / torch, horizon < 1, phase0 outside 0 .. p-1, D without d, ndcnt outside 0 .. nd, tol <= 0,
    max_iter < 1, penalty without D or with an entry <= 0 or NaN (0 is legal beside a penalty2 > 0), penalty2 without D, negative, non-finite, NaN or non-zero
    on a hard row, r or necnt without J, a terminal that is neither None, 'constraint' nor an array,
    terminal_rhs without terminal; NotImplementedError: n > 64, (nx, nu, nd) beyond the 160 KB LDS layout (lds_layout; with a penalty the soft layout, with J or terminal lds_layout(ne=))."""
    return _step('mpc_qp_batch', A, B, H, X0, horizon, phase0, D, d, ndcnt, q, Pf, tol, max_iter, return_traj, offset, qf, terminal_rhs, penalty, J, r, necnt,
                 terminal, penalty2, guess, guess_shift, warm_floor, warm_call)


def _step(who, A, B, H, X0, horizon, phase0=0, D=None, d=None, ndcnt=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER, return_traj=True, offset=None, qf=None,
          terminal_rhs=None, penalty=None, J=None, r=None, necnt=None, terminal=None, penalty2=None, guess=None, guess_shift=0, warm_floor=WARM_FLOOR,
          force_warm=False):
    """mpc_qp_batch under the name `who`; force_warm: through the warm entry also without a warm-start keyword (the dict then always holds `warm`)."""
    o = _run(who, A, B, H, X0, horizon, 1, phase0, D, d, ndcnt, q, Pf, tol, max_iter, False, return_traj, penalty, J, r, necnt, terminal, offset, qf,
             terminal_rhs, penalty2=penalty2, guess=guess, guess_shift=guess_shift, warm_floor=warm_floor, force_warm=force_warm)
    out = dict(u0=o['U0'], X=o['Xol'], U=o['Uol'], lam=o['Lam'], nact=o['nact'][..., 0], hres=o['hres'][..., 0], x1=o['XT'], info=o['info'])
    if penalty is not None or penalty2 is not None:
        out.update(eps=o['Eol'], nviol=o['nviol'][..., 0])
    if 'eres' in o:
        out.update(nu=o['Nu'], nu_term=o['NuT'], eres=o['eres'][..., 0])
    if 'warmlog' in o:
        out['warm'] = o['warmlog'][..., 0]
    out.update({k: o[k] for k in INFO_FIELDS})
    return out


@_hidden_keywords
def mpc_closed_loop_batch(A, B, H, X0, horizon, steps, phase0=0, D=None, d=None, ndcnt=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER, return_traj=True,
                          offset=None, qf=None, terminal_rhs=None, plant=None, disturbance=None, penalty=None, J=None, r=None, necnt=None, terminal=None,
                          penalty2=None, guess=None, guess_shift=0, warm=False, warm_floor=WARM_FLOOR,
                          warm_call=False):
    """The receding-horizon loop: at t = 0 .. steps-1 the QP of mpc_qp_batch from phase (phase0 + t) mod p, cold-started (or warm: below), u_0 applied, x <- A_k x + B_k u_0 (the
    linear plant, as closed_loop_batch does), all steps in one launch.  Arguments as mpc_qp_batch.

    Returns dict: X [nb,ns,steps+1,nx], U [nb,ns,steps,nu] (None with return_traj=False), iters, nact [nb,ns,steps] int32, hres [nb,ns,steps], XT [nb,ns,nx],
    u0 [nb,ns,nu] (the first input of step 0) and the info fields of mpc_qp_batch (steps: steps finished).  An instance that fails at step t (status 1, 2, 3)
    keeps what it logged before: U, hres from t on, X from t + 1 on and XT are NaN, nact from t on and iters beyond t are -1.  X, U and the per-step logs are
    permuted views of time-major arrays.  With penalty (as in mpc_qp_batch) the dict gains nviol [nb,ns,steps] int32 (-1 from a failed step on); hres > 0
    at a step whose applied stage violates a soft row.  With J or terminal (as in mpc_qp_batch) the dict gains eres [nb,ns,steps] = max|J z_0 - r| of the
    applied stage (NaN from a failed step on).
    offset, qf, terminal_rhs as in mpc_qp_batch.  plant = (Ap, Bp) or (Ap, Bp, cp) with the shapes of A, B, offset: the plant step is
    x_{t+1} = Ap_k x_t + Bp_k u_0 + cp_k + W_t, k = (phase0 + t) mod p (default: the model; a cp left out is the model's offset); disturbance W
    [nb,ns,steps,nx], which the controller does not know about.  hres, eres, nact, nviol stay figures of the applied stage of the model's QP.  A non-finite
    W_t (or plant entry) makes x_{t+1} non-finite: the instance ends with status 3 at step t + 1, X[t + 1] holds that state.  With any of the five the dict
    also holds eres.  penalty2 as in mpc_qp_batch (the dict gains nviol and eres).
    warm=False, guess=None, guess_shift=0, warm_floor=1e-2 (keyword-only, not listed by inspect.signature): with warm=True every step t > 0 starts from the
    iterate of step t - 1 shifted by one stage, in place in the workspace of the launch; guess (as in mpc_qp_batch) is the start of step 0.  The fallbacks of
    mpc_qp_batch hold per step: a warm-started step that ends with status 1 or 2 is solved again cold within the step and iters (with it iters_total,
    iters_max, which may exceed max_iter, and pivmin) counts both attempts.  A call
    that passes any of these keywords, whatever the value, returns `warm` [nb,ns,steps] int32 in addition (0 cold, 1 the warm start delivered the step, 2 the cold restart delivered it,
    -1 from a failed step on).  ValueError: shapes, mixed numpy / torch, terminal_rhs without terminal, a plant that is not a tuple of 2 or 3."""
    o = _run('mpc_closed_loop_batch', A, B, H, X0, horizon, steps, phase0, D, d, ndcnt, q, Pf, tol, max_iter, return_traj, False, penalty, J, r, necnt, terminal,
             offset, qf, terminal_rhs, plant, disturbance, penalty2, guess, guess_shift, warm, warm_floor, warm_call)
    out = dict(X=o['X'], U=o['U'], iters=o['iters'], nact=o['nact'], hres=o['hres'], XT=o['XT'], u0=o['U0'], info=o['info'])
    if penalty is not None or penalty2 is not None:
        out['nviol'] = o['nviol']
    if 'eres' in o:
        out['eres'] = o['eres']
    if 'warmlog' in o:
        out['warm'] = o['warmlog']
    out.update({k: o[k] for k in INFO_FIELDS})
    return out


def _stack_eq(who, p, nx, n, J, r, terminal):
    """J, r (single arrays or lists of p, None entries: no rows at that stage) and terminal (None, 'constraint', one matrix [nt,nx] or a list of p) -> dict J,
    r, necnt, terminal of one problem."""
    out = dict(J=None, r=None, necnt=None, terminal=None)
    if J is None and r is not None:
        raise ValueError('{}: r describes the rows of J, which is None'.format(who))
    if J is not None:
        Jl = [None if m is None else np.atleast_2d(_to_array(m)).astype(np.float64) for m in (J if isinstance(J, (list, tuple)) else [J] * p)]
        rl = [None] * p if r is None else [None if v is None else _to_array(v).astype(np.float64).reshape(-1) for v in (r if isinstance(r, (list, tuple)) else [r] * p)]
        if len(Jl) != p or len(rl) != p:
            raise ValueError('{}: J, r must be single arrays or lists of p = {} (None: no rows at that stage)'.format(who, p))
        cnts = [0 if m is None else m.shape[0] for m in Jl]
        for k in range(p):
            if (Jl[k] is not None and Jl[k].shape[1] != n) or (rl[k] is not None and rl[k].shape != (cnts[k],)):
                raise ValueError('{}: J[{}] (rows, nx + nu = {}) with r[{}] (rows) or None expected'.format(who, k, n, k))
        ne = max(cnts)
        if ne:
            Js = np.zeros((1, p, ne, n)); rs = np.zeros((1, p, ne))
            for k in range(p):
                if cnts[k]:
                    Js[0, k, :cnts[k]] = Jl[k]
                    if rl[k] is not None:
                        rs[0, k, :cnts[k]] = rl[k]
            out.update(J=Js, r=rs, necnt=np.asarray([cnts], np.int32))
    if isinstance(terminal, str):
        out['terminal'] = terminal                                          # (checked by the batch call)
    elif terminal is not None:
        Tl = [np.atleast_2d(_to_array(m)).astype(np.float64) for m in (terminal if isinstance(terminal, (list, tuple)) else [terminal] * p)]
        if len(Tl) != p or any(m.shape != Tl[0].shape or m.shape[1] != nx for m in Tl):
            raise ValueError('{}: terminal must be \'constraint\', one matrix [nt, nx = {}] or a list of p = {} of them'.format(who, nx, p))
        out['terminal'] = np.ascontiguousarray(np.stack(Tl)[None])
    return out


def _stack_affine(who, p, nx, nu, terminal, offset, qf, terminal_rhs, plant=None, disturbance=None, steps=None):
    """offset, qf, terminal_rhs (single vectors or lists of p), plant ((Ap, Bp[, cp]), each a single array or a list of p), disturbance [steps, nx] -> the
    keyword arguments of the batch calls for one problem and one state (only those that are given)."""
    out = {}

    def vecs(name, v, m):
        vl = [_to_array(x).astype(np.float64).reshape(-1) for x in (v if isinstance(v, (list, tuple)) else [v] * p)]
        if len(vl) != p or any(x.shape != (m,) for x in vl):
            raise ValueError('{}: {} must be one vector of {} entries or a list of p = {} of them'.format(who, name, m, p))
        return np.ascontiguousarray(np.stack(vl)[None])

    def mats(name, v, rows, cols):
        ml = [np.atleast_2d(_to_array(x)).astype(np.float64) for x in (v if isinstance(v, (list, tuple)) else [v] * p)]
        if len(ml) != p or any(x.shape != (rows, cols) for x in ml):
            raise ValueError('{}: {} must be one matrix [{}, {}] or a list of p = {} of them'.format(who, name, rows, cols, p))
        return np.ascontiguousarray(np.stack(ml)[None])
    if offset is not None:
        out['offset'] = vecs('offset', offset, nx)
    if qf is not None:
        out['qf'] = vecs('qf', qf, nx)
    if terminal_rhs is not None:
        if terminal is None:
            raise ValueError('{}: terminal_rhs describes the rows of terminal, which is None'.format(who))
        nt = nx if isinstance(terminal, str) else int(terminal.shape[2])
        out['terminal_rhs'] = vecs('terminal_rhs', terminal_rhs, nt)
    if plant is not None:
        if not isinstance(plant, tuple) or len(plant) not in (2, 3):
            raise ValueError('{}: plant must be a tuple (Ap, Bp) or (Ap, Bp, cp), got {!r}'.format(who, type(plant).__name__ if not isinstance(plant, tuple) else len(plant)))
        pl = (mats('plant[0]', plant[0], nx, nx), mats('plant[1]', plant[1], nx, nu))
        out['plant'] = pl + ((vecs('plant[2]', plant[2], nx),) if len(plant) == 3 and plant[2] is not None else ())
    if disturbance is not None:
        W = np.atleast_2d(_to_array(disturbance)).astype(np.float64)
        if W.shape != (int(steps), nx):
            raise ValueError('{}: disturbance [steps, nx] = [{}, {}] expected, got {}'.format(who, int(steps), nx, W.shape))
        out['disturbance'] = np.ascontiguousarray(W[None, None])
    return out


def _stack_guess(who, guess):
    """guess of the reference calling style -> dict(guess=) of the batch calls: its arrays gain the two leading axes of one problem and one state."""
    out = dict(guess=None)
    if guess is not None:
        if not isinstance(guess, dict):
            raise ValueError('{}: guess must be a dict with X, U, lam (and eps, nu, nu_term where the problem has them), got {}'.format(who, type(guess).__name__))
        out['guess'] = {k: None if guess.get(k) is None else np.ascontiguousarray(_to_array(guess[k]).astype(np.float64)[None, None]) for k in GUESS_KEYS}
    return out


def _stack_one(who, A, B, Q, R, N, x0, D, d, q, Pf, penalty=None, penalty2=None):
    """The reference's calling style -> batched arrays of one problem and one state."""
    try:
        As, Bs, Hs, _ = lqr._stack_stages(A, B, Q, R, N)
    except ValueError as e:
        raise ValueError(str(e).replace('periodic_lqr', who)) from None
    p, nx, nu = As.shape[1], As.shape[2], Bs.shape[3]
    n = nx + nu
    x = _to_array(x0).astype(np.float64).reshape(-1)
    if x.shape != (nx,):
        raise ValueError('{}: x0 must hold nx = {} entries, got {}'.format(who, nx, _to_array(x0).shape))
    Ds = ds = cnt = pens = pens2 = None
    if (D is None) != (d is None):
        raise ValueError('{}: D and d come together (the rows D z <= d)'.format(who))
    if D is None and penalty is not None:
        raise ValueError('{}: penalty describes the rows of D, which is None'.format(who))
    if D is None and penalty2 is not None:
        raise ValueError('{}: penalty2 describes the rows of D, which is None'.format(who))
    if D is not None:
        Dl = [None if m is None else np.atleast_2d(_to_array(m)).astype(np.float64) for m in (D if isinstance(D, (list, tuple)) else [D] * p)]
        dl = [None if v is None else _to_array(v).astype(np.float64).reshape(-1) for v in (d if isinstance(d, (list, tuple)) else [d] * p)]
        if len(Dl) != p or len(dl) != p:
            raise ValueError('{}: D, d must be single arrays or lists of p = {} (None: no rows at that stage)'.format(who, p))
        cnts = [0 if m is None else m.shape[0] for m in Dl]
        for k in range(p):
            if (Dl[k] is None) != (dl[k] is None) or (Dl[k] is not None and (Dl[k].shape[1] != n or dl[k].shape != (cnts[k],))):
                raise ValueError('{}: D[{}] (rows, nx + nu = {}) with d[{}] (rows) expected'.format(who, k, n, k))
        nd = max(cnts)
        if nd:
            Ds = np.zeros((1, p, nd, n)); ds = np.zeros((1, p, nd)); cnt = np.asarray([cnts], np.int32)
            for k in range(p):
                if cnts[k]:
                    Ds[0, k, :cnts[k]] = Dl[k]; ds[0, k, :cnts[k]] = dl[k]
        if penalty is not None:
            pl = [None if v is None else _to_array(v).astype(np.float64).reshape(-1) for v in (penalty if isinstance(penalty, (list, tuple)) else [penalty] * p)]
            if len(pl) != p or any(v is not None and v.shape != (cnts[k],) for k, v in enumerate(pl)):
                raise ValueError('{}: penalty must be one vector or a list of p = {} vectors (None: a stage of hard rows) with one entry per row of D'.format(who, p))
            if penalty2 is None and any(v is not None and not (v > 0).all() for v in pl):
                raise ValueError('{}: penalty > 0 expected in every entry (inf: a hard row)'.format(who))
            if nd:
                pens = np.full((1, p, nd), np.inf)
                for k in range(p):
                    if pl[k] is not None:
                        pens[0, k, :cnts[k]] = pl[k]
        if penalty2 is not None:
            zl = [None if v is None else _to_array(v).astype(np.float64).reshape(-1) for v in (penalty2 if isinstance(penalty2, (list, tuple)) else [penalty2] * p)]
            if len(zl) != p or any(v is not None and v.shape != (cnts[k],) for k, v in enumerate(zl)):
                raise ValueError('{}: penalty2 must be one vector or a list of p = {} vectors (None: no quadratic penalty at that stage) with one entry per row '
                                 'of D'.format(who, p))
            if nd:
                pens2 = np.zeros((1, p, nd))
                if pens is None:                                            # penalty=None: every row with Z > 0 pure quadratic, the others hard
                    pens = np.full((1, p, nd), np.inf)
                    for k in range(p):
                        if zl[k] is not None:
                            pens[0, k, :cnts[k]] = np.where(zl[k] > 0, 0.0, np.inf)
                for k in range(p):
                    if zl[k] is not None:
                        pens2[0, k, :cnts[k]] = zl[k]
                        _check_penalty2(who, pens[0, k, :cnts[k]], zl[k])
    qs = None
    if q is not None:
        ql = [_to_array(v).astype(np.float64).reshape(-1) for v in (q if isinstance(q, (list, tuple)) else [q] * p)]
        if len(ql) != p or any(v.shape != (n,) for v in ql):
            raise ValueError('{}: q must be one vector of nx + nu = {} entries or a list of p = {} of them'.format(who, n, p))
        qs = np.ascontiguousarray(np.stack(ql)[None])
    try:
        Pfs = lqr._stack_weights(Pf, p, nx, 'Pf')
    except ValueError as e:
        raise ValueError(str(e).replace('horizon_lqr', who)) from None
    out = dict(D=Ds, d=ds, ndcnt=cnt, q=qs, Pf=Pfs, penalty=pens)
    if penalty2 is not None:
        out['penalty2'] = pens2
    return As, Bs, Hs, np.ascontiguousarray(x[None, None]), out


@_hidden_keywords
def mpc_step(A, B, Q, R, N, x0, horizon, phase0=0, D=None, d=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER, offset=None, qf=None, terminal_rhs=None, penalty=None,
             J=None, r=None, terminal=None, penalty2=None, guess=None, guess_shift=0, warm_floor=WARM_FLOOR, warm_call=False):
    """One MPC step of one model in the reference's calling style: A, B, Q, R, N (the cross term) single matrices (p = 1) or lists of length p as in horizon_lqr,
    D, d the rows D_k [x; u] <= d_k (single arrays or lists of p; None entries: no rows at that stage), q, Pf likewise.  Returns (u0, X [horizon+1,nx],
    U [horizon,nu], lam [horizon,nd], info dict).  penalty: the weights of the soft rows, one vector (every stage) or a list of p vectors, one entry per row of
    D_k; np.inf entries and None stages are hard.  With it info gains 'eps' [horizon,nd] (the slacks) and 'nviol'.  J, r: the equality rows J_k [x; u] = r_k
    (single arrays or lists of p, None entries: no rows at that stage; r None: zero); terminal: 'constraint' (x_N = 0), one matrix Tx [nt,nx] or a list of p
    (Tx x_N = 0).  With them info gains 'nu' [horizon,ne], 'nu_term' [nt] and 'eres'.  offset, qf, terminal_rhs: the vectors of the affine problem
    (mpc_qp_batch), one vector each or a list of p.  penalty2: the quadratic weights of the slacks (mpc_qp_batch), one vector or a list of p vectors like
    penalty; without penalty the rows with Z > 0 are pure quadratic and the others hard.  guess, guess_shift=0, warm_floor=1e-2 (keyword-only): the warm start
    of mpc_qp_batch for one model; guess is a dict with X [horizon+1,nx], U [horizon,nu], lam [horizon,nd] and eps, nu, nu_term where the problem has them: the
    X, U, lam this function returned and the entries of its info.  With any of the three info gains 'warm'.  RuntimeError when the solve did not converge (an
    infeasible problem)."""
    who = 'mpc_step'
    As, Bs, Hs, X0, kw = _stack_one(who, A, B, Q, R, N, x0, D, d, q, Pf, penalty, penalty2)
    kw.update(_stack_eq(who, As.shape[1], As.shape[2], As.shape[2] + Bs.shape[3], J, r, terminal))
    kw.update(_stack_affine(who, As.shape[1], As.shape[2], Bs.shape[3], kw['terminal'], offset, qf, terminal_rhs))
    if warm_call:
        kw.update(_stack_guess(who, guess), guess_shift=guess_shift, warm_floor=warm_floor)
    res = mpc_qp_batch(As, Bs, Hs, X0, horizon, phase0, tol=tol, max_iter=max_iter, **kw)
    st = int(res['status'][0, 0])
    if st != 0:
        raise RuntimeError('{}: the solve ended with status {} ({}) after {} iterations'.format(who, st, STATUS_NAMES.get(st), int(res['iters_total'][0, 0])))
    return res['u0'][0, 0], res['X'][0, 0], res['U'][0, 0], res['lam'][0, 0], {k: res[k][0, 0] for k in INFO_FIELDS + ('nact', 'hres') + (('eps', 'nviol') if 'eps' in res else ()) + (('nu', 'nu_term', 'eres') if 'nu' in res else ()) + (('warm',) if 'warm' in res else ())}


@_hidden_keywords
def mpc_closed_loop_sim(A, B, Q, R, N, x0, horizon, steps, phase0=0, D=None, d=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER, offset=None, qf=None,
                        terminal_rhs=None, plant=None, disturbance=None, penalty=None, J=None, r=None, terminal=None, penalty2=None, guess=None, guess_shift=0,
                        warm=False, warm_floor=WARM_FLOOR, warm_call=False):
    """The reference's closed_loop_sim with the inequality-constrained tracking MPC in the loop and the linear plant, one model in the calling style of mpc_step.
    Returns the reference's log: {'x': steps + 1 states, 'u': steps inputs, 'l': steps stage costs 1/2 z' H_k z + q_k' z, 'h': steps arrays d_k - D_k [x_t; u_t]
    (>= 0 when the rows hold; empty at a stage without rows)} and 'iters', 'nact'.  With penalty (as in mpc_step) 'h' stays d - D z (negative on a violated soft
    row), 'usc' holds the slack of the applied step, max(0, D z - d) on the soft rows and 0 on the hard ones (the reference's usc), and 'nviol' the count of the
    solver.  With J, r, terminal (as in mpc_step) the log gains 'eres': max|J_k [x_t; u_t] - r_k| of every step.  offset, qf, terminal_rhs as in mpc_step; plant = (Ap, Bp) or (Ap, Bp, cp), each a single
    array or a list of p, and disturbance [steps, nx]: the plant of the loop, x_{t+1} = Ap_k x_t + Bp_k u_t + cp_k + W_t (mpc_closed_loop_batch).
    penalty2 as in mpc_step: 'usc' covers the rows of both kinds (L1, L1 + L2 and pure quadratic).  warm=False, guess, guess_shift, warm_floor (keyword-only,
    mpc_closed_loop_batch; guess as in mpc_step): with warm=True every step after the first starts from the shifted iterate of the step before, as the
    reference's Pmpc.step does; with any of the four the log gains 'warm' (the code of every step).  RuntimeError when a step did not converge."""
    who = 'mpc_closed_loop_sim'
    As, Bs, Hs, X0, kw = _stack_one(who, A, B, Q, R, N, x0, D, d, q, Pf, penalty, penalty2)
    kw.update(_stack_eq(who, As.shape[1], As.shape[2], As.shape[2] + Bs.shape[3], J, r, terminal))
    kw.update(_stack_affine(who, As.shape[1], As.shape[2], Bs.shape[3], kw['terminal'], offset, qf, terminal_rhs, plant, disturbance, steps))
    if warm_call:
        kw.update(_stack_guess(who, guess), guess_shift=guess_shift, warm=warm, warm_floor=warm_floor)
    res = mpc_closed_loop_batch(As, Bs, Hs, X0, horizon, steps, phase0, tol=tol, max_iter=max_iter, **kw)
    st = int(res['status'][0, 0])
    if st != 0:
        raise RuntimeError('{}: step {} of {} ended with status {} ({})'.format(who, int(res['steps'][0, 0]), int(steps), st, STATUS_NAMES.get(st)))
    T, p = int(steps), As.shape[1]
    X, U = res['X'][0, 0], res['U'][0, 0]
    log = {'x': [X[t].copy() for t in range(T + 1)], 'u': [U[t].copy() for t in range(T)], 'l': [], 'h': [], 'iters': [int(v) for v in res['iters'][0, 0]],
           'nact': [int(v) for v in res['nact'][0, 0]]}
    for t in range(T):
        k = (int(phase0) + t) % p
        z = np.concatenate([X[t], U[t]])
        Hk = (Hs[0, k] + Hs[0, k].T) / 2
        log['l'].append(float(0.5 * z @ Hk @ z + (kw['q'][0, k] @ z if kw['q'] is not None else 0.0)))
        m = int(kw['ndcnt'][0, k]) if kw['D'] is not None else 0
        log['h'].append(kw['d'][0, k, :m] - kw['D'][0, k, :m] @ z if m else np.zeros(0))
        if kw['penalty'] is not None:
            log.setdefault('usc', []).append(np.where(np.isfinite(kw['penalty'][0, k, :m]), np.maximum(0.0, -log['h'][-1]), 0.0))
    if kw['penalty'] is not None:
        log['nviol'] = [int(v) for v in res['nviol'][0, 0]]
    if 'eres' in res:
        log['eres'] = [float(v) for v in res['eres'][0, 0]]
    if 'warm' in res:
        log['warm'] = [int(v) for v in res['warm'][0, 0]]
    return log


def mpc_closed_loop_plant(A, B, H, X0, horizon, steps, plant, phase0=0, warm=True, **problem):
    """The receding-horizon loop of mpc_closed_loop_batch against ANY plant (the reference's closed_loop_sim(F=...) on a plant that is not linear): at
    t = 0 .. steps-1 one launch of mpc_qp_batch from phase (phase0 + t) mod p on the current states, then X <- plant(t, X, U0) with X [nb,ns,nx] and
    U0 [nb,ns,nu] of the array kind of the call (numpy or torch), returning the next states [nb,ns,nx] of the same kind.  warm=True: the step after a solved
    one starts from its solution, guess_shift=1 (the rule of mpc_qp_batch with its fallbacks; an instance that failed returns NaN and drags no other along).
    problem: the keyword arguments of mpc_qp_batch (D, d, ndcnt, q, Pf, tol, max_iter, offset, qf, terminal_rhs, penalty, J, r, necnt, terminal, penalty2,
    warm_floor, and guess / guess_shift for step 0); disturbance= of mpc_closed_loop_batch has no place here: the callback is the plant.

    Returns the keys of mpc_closed_loop_batch: X [nb,ns,steps+1,nx], U [nb,ns,steps,nu], iters, nact [nb,ns,steps] int32, hres [nb,ns,steps], XT, u0, the info
    fields (status: of the step that failed, 0 otherwise; steps: steps finished; iters_total, iters_max over the finished steps and the failed one; mu, rp,
    rd, pivmin of the last step that ran; info [nb,ns,8] assembled from them), nviol with penalty or penalty2, eres where mpc_qp_batch returns it, and warm
    [nb,ns,steps] int32.  An instance that fails at step t keeps what it logged before: U, hres, eres from t on, X from t + 1 on and XT are NaN, nact, nviol
    and warm from t on and iters beyond t are -1 (its state is NaN from then on, so its later launches end at once with status 3 and are not logged).
    With a linear plant(t, X, U0) = A_k X + B_k U0 this is mpc_closed_loop_batch(warm=True): the same starts, so the same iters and warm codes in practice; the
    values agree to rounding, not bit for bit -- the callback's matrix products are not the kernel's fused sums.  ValueError: as mpc_qp_batch, a plant that
    is not callable or returns another shape or kind, return_traj=False (the guess of the next step is the trajectory)."""
    who = 'mpc_closed_loop_plant'
    if not callable(plant):
        raise ValueError('{}: plant must be a callable plant(t, X, U0) -> X_next, got {!r}'.format(who, type(plant).__name__))
    for k in ('disturbance', 'return_traj'):
        if k in problem:
            raise ValueError('{}: {} has no place here (the callback is the plant; the trajectory of a step is the guess of the next)'.format(who, k))
    if isinstance(warm, (bool, np.bool_)) is False:
        raise ValueError('{}: warm must be a bool, got {!r}'.format(who, warm))
    T, _ = _cl._validate_steps(who, steps, phase0, int(A.shape[1]) if hasattr(A, 'shape') and len(A.shape) == 4 else 1)
    p = int(A.shape[1])
    use_torch = lqr._is_torch(A)
    if use_torch:
        import torch
        stack, i32 = (lambda xs: torch.stack(xs, dim=2)), (lambda x: x.to(torch.int32))
        full = lambda like, v: torch.full_like(like, v)
        where = torch.where
    else:
        stack, i32 = (lambda xs: np.stack(xs, axis=2)), (lambda x: x.astype(np.int32))
        full = lambda like, v: np.full_like(like, v)
        where = np.where
    guess, shift = problem.pop('guess', None), problem.pop('guess_shift', 0)
    floor = problem.pop('warm_floor', WARM_FLOOR)
    X, logs = [X0], {k: [] for k in ('U', 'iters', 'nact', 'hres', 'nviol', 'eres', 'warm')}
    alive = None                                                            # [nb,ns] bool: every step so far converged
    for t in range(T):
        o = _step(who, A, B, H, X[-1], horizon, (int(phase0) + t) % p, guess=guess, guess_shift=shift, warm_floor=floor, force_warm=True, **problem)
        ok = o['status'] == 0
        if alive is None:
            alive, u0 = ok | ~ok, o['u0']
            status, nsteps, it_total, it_max = o['status'] * 0, o['status'] * 0, o['status'] * 0, o['status'] * 0
            last = {k: o[k] for k in ('mu', 'rp', 'rd', 'pivmin')}
        ran, alive = alive, alive & ok                                       # the instances for which step t is a real one; those that solved it too
        status = where(ran & ~ok, o['status'], status)
        nsteps = nsteps + i32(alive)
        its = where(ran, o['iters_total'], o['iters_total'] * 0)
        it_total, it_max = it_total + its, where(its > it_max, its, it_max)
        last = {k: where(ran, o[k], last[k]) for k in last}
        m1 = full(o['nact'], -1)
        logs['U'].append(o['u0']); logs['hres'].append(where(alive, o['hres'], full(o['hres'], float('nan'))))
        logs['iters'].append(where(ran, o['iters_total'], m1)); logs['nact'].append(where(alive, o['nact'], m1))
        logs['warm'].append(where(alive, o['warm'], m1))
        if 'nviol' in o:
            logs['nviol'].append(where(alive, o['nviol'], m1))
        logs['eres'].append(where(alive, o['eres'], full(o['eres'], float('nan'))))
        Xn = plant(t, X[-1], o['u0'])
        if lqr._is_torch(Xn) != use_torch or not hasattr(Xn, 'shape') or tuple(Xn.shape) != tuple(X0.shape):
            raise ValueError('{}: plant(t, X, U0) must return the next states {} of the kind of X, got {}'.format(
                who, tuple(X0.shape), tuple(Xn.shape) if hasattr(Xn, 'shape') else type(Xn).__name__))
        X.append(where(alive[..., None], Xn, full(Xn, float('nan'))))
        if warm:
            guess, shift = {k: o.get(k) for k in GUESS_KEYS}, 1
        else:
            guess, shift = None, 0
    out = dict(X=stack(X), U=stack(logs['U']), iters=stack(logs['iters']), nact=stack(logs['nact']), hres=stack(logs['hres']), XT=X[-1], u0=u0)
    if logs['nviol']:
        out['nviol'] = stack(logs['nviol'])
    out.update(eres=stack(logs['eres']), warm=stack(logs['warm']))
    f64 = (lambda x: x.to(X0.dtype)) if use_torch else (lambda x: x.astype(np.float64))
    fields = dict(status=status, steps=nsteps, iters_total=it_total, iters_max=it_max, mu=last['mu'], rp=last['rp'], rd=last['rd'], pivmin=last['pivmin'])
    out['info'] = stack([f64(fields[k]) for k in INFO_FIELDS])
    out.update(fields)
    return out


def about_reference(A, B, H, xref, uref, q=None, Pf=None, D=None, d=None, J=None, r=None, terminal=None):
    """A problem in DEVIATION coordinates (the arguments of mpc_qp_batch: A [nb,p,nx,nx], B [nb,p,nx,nu], H [nb,p,n,n], q [nb,p,n], Pf [nb,p,nx,nx], D, d, J, r,
    terminal as there) and a p-periodic reference xref [nb,p,nx], uref [nb,p,nu] -> the keyword arguments of the same problem in ABSOLUTE coordinates
    w = dw + wref, wref_k = [xref_k; uref_k], H used as (H + H') / 2, likewise Pf:
        offset_k = xref_{(k+1) % p} - A_k xref_k - B_k uref_k       (zero when the reference is a trajectory of the model),
        q_k - H_k wref_k,   d_k + D_k wref_k,   r_k + J_k wref_k,   qf_k = -Pf_k xref_k,   terminal_rhs_k = Tx_k xref_k  (xref_k for terminal='constraint').
    Returns a dict with offset, q, and, where the argument is given, Pf, qf, D, d, J, r, terminal, terminal_rhs: pass it as **kwargs next to A, B, H and the
    ABSOLUTE X0 (and ndcnt, necnt, penalty, penalty2, which do not change: penalty2 passes through like penalty).  The solution is the deviation solution plus the reference with the same multipliers; the
    cost differs by a constant.  Host-side numpy or torch (all arguments of one kind), no kernel.  A producer of xref, uref is tunempc_amd.periodic_qp:
    X[:, :p], U[:, :p] of periodic_qp_batch are what this function takes as xref, uref."""
    who = 'about_reference'
    Tx = terminal if hasattr(terminal, 'shape') else None
    if terminal is not None and Tx is None and not (isinstance(terminal, str) and terminal == 'constraint'):
        raise ValueError("{}: terminal must be None, 'constraint' or an array [nb, p, nt, nx], got {!r}".format(who, terminal))
    named = [('A', A), ('B', B), ('H', H), ('xref', xref), ('uref', uref)] + [(nm, x) for nm, x in (('q', q), ('Pf', Pf), ('D', D), ('d', d), ('J', J), ('r', r),
                                                                                                      ('terminal', Tx)) if x is not None]
    use_torch = [lqr._is_torch(x) for _, x in named]
    if any(use_torch) != all(use_torch) or not all(hasattr(x, 'shape') for _, x in named):
        raise ValueError('{}: all arguments numpy arrays or all torch tensors expected'.format(who))
    if len(A.shape) != 4 or A.shape[2] != A.shape[3] or len(B.shape) != 4 or tuple(B.shape[:3]) != tuple(A.shape[:3]):
        raise ValueError('{}: A [nb, p, nx, nx], B [nb, p, nx, nu] expected, got {}, {}'.format(who, tuple(A.shape), tuple(B.shape)))
    nb, p, nx, _ = (int(v) for v in A.shape)
    nu = int(B.shape[3])
    n = nx + nu
    if (D is None) != (d is None):
        raise ValueError('{}: D and d come together (the rows D z <= d)'.format(who))
    if J is None and r is not None:
        raise ValueError('{}: r describes the rows of J, which is None'.format(who))
    for nm, x, shape in (('H', H, (nb, p, n, n)), ('xref', xref, (nb, p, nx)), ('uref', uref, (nb, p, nu)), ('q', q, (nb, p, n)), ('Pf', Pf, (nb, p, nx, nx)),
                         ('D', D, (nb, p, None, n)), ('J', J, (nb, p, None, n)), ('terminal', Tx, (nb, p, None, nx))):
        if x is not None and (len(x.shape) != len(shape) or any(b is not None and int(a) != b for a, b in zip(x.shape, shape))):
            raise ValueError('{}: {} {} expected, got {}'.format(who, nm, tuple('any' if v is None else v for v in shape), tuple(x.shape)))
    if D is not None and tuple(d.shape) != tuple(D.shape[:3]):
        raise ValueError('{}: d {} expected, got {}'.format(who, tuple(D.shape[:3]), tuple(d.shape)))
    if r is not None and tuple(r.shape) != tuple(J.shape[:3]):
        raise ValueError('{}: r {} expected, got {}'.format(who, tuple(J.shape[:3]), tuple(r.shape)))
    if use_torch[0]:
        import torch
        cat, roll = (lambda a, b: torch.cat([a, b], dim=-1)), (lambda x: torch.roll(x, -1, dims=1))
    else:
        cat, roll = (lambda a, b: np.concatenate([a, b], axis=-1)), (lambda x: np.roll(x, -1, axis=1))
    mv = lambda M, v: (M @ v[..., None])[..., 0]
    tr = lambda M: M.transpose(-1, -2) if use_torch[0] else np.swapaxes(M, -1, -2)
    w = cat(xref, uref)
    out = dict(offset=roll(xref) - mv(A, xref) - mv(B, uref))
    Hw = 0.5 * (mv(H, w) + mv(tr(H), w))
    out['q'] = -Hw if q is None else q - Hw
    if Pf is not None:
        out.update(Pf=Pf, qf=-0.5 * (mv(Pf, xref) + mv(tr(Pf), xref)))
    if D is not None:
        out.update(D=D, d=d + mv(D, w))
    if J is not None:
        out.update(J=J, r=mv(J, w) if r is None else r + mv(J, w))
    if terminal is not None:
        out.update(terminal=terminal, terminal_rhs=xref + 0.0 if Tx is None else mv(Tx, xref))
    return out


def slack_penalty(lam_h, active_set=None, slack_flag='active', factor=1e3):
    """The reference's rule for the weights of the soft rows (preprocessing.add_mpc_slacks), restated on the host: lam_h [N, nh] the multipliers of h(x, u) >= 0
    along the optimal periodic orbit (<= 0 where a row is active, the reference's sign), active_set a list of N index lists (the rows active at each stage).
    slack_flag 'active': the rows that are active at some stage; 'all': every row; 'none': no row.  Returns penalty [nh]: factor max_k(-lam_h[k, i]) on the selected
    rows, inf elsewhere (a selected row whose multiplier is 0 everywhere stays hard: a weight of 0 is no penalty).  Pass it as penalty= (one vector for every stage)."""
    lam = np.atleast_2d(_to_array(lam_h)).astype(np.float64)
    nh = lam.shape[1]
    if slack_flag not in ('active', 'all', 'none'):
        raise ValueError("slack_penalty: slack_flag must be 'active', 'all' or 'none', got {!r}".format(slack_flag))
    if not float(factor) > 0.0:
        raise ValueError('slack_penalty: factor > 0 expected, got {!r}'.format(factor))
    if slack_flag == 'active' and active_set is None:
        raise ValueError("slack_penalty: slack_flag 'active' needs the active set")
    out = np.full(nh, np.inf)
    if slack_flag == 'none':
        return out
    sel = range(nh) if slack_flag == 'all' else sorted({int(i) for a in active_set for i in a})
    if any(i < 0 or i >= nh for i in sel):
        raise ValueError('slack_penalty: the active set names a row outside 0 .. {}'.format(nh - 1))
    for i in sel:
        w = float(factor) * float(np.max(-lam[:, i]))
        if w > 0.0:
            out[i] = w
    return out


# ----------------------------------------------------------------------------- the local gain of a solved step and its certificate
GAIN_STATUS_NAMES = {0: 'Done', 2: 'SingularS', 3: 'NonFinite', 5: 'NoFeasibleSubspace'}
CLASS_NAMES = {0: 'free', 1: 'equality', 2: 'quadratic'}


def gain_lds_bytes(nx, nu, nd=0, ne=0):
    """mpc_qp_gain_lds_doubles of csrc/tmpc_mpc_qp_gain.h restated: the layout of the constraint-to-go stage (lqr_ctg_lds) with room for ne + nd rows, then
    nd + 1 doubles for the classes -> bytes of LDS of a workgroup."""
    nx, nu, nr = int(nx), int(nu), int(ne) + int(nd)
    n = nx + nu
    nbd, ms = min(nu, nr + nx), max(nr + nx, nu)
    ld, ldp, ldc = (n + nbd) | 1, nx | 1, n | 1
    total = nx * ld + nx * ldp + max(nx, nu + nbd) * ld + (n + nbd) * ld + 2 * ms * ldc + 2 * nx * ldp + 16
    return 8 * (total + int(nd) + 1)


def mpc_qp_gain_batch(A, B, H, sol, horizon, phase0=0, D=None, d=None, ndcnt=None, Pf=None, penalty=None, penalty2=None, J=None, necnt=None, terminal=None,
                      active=None, rank_tol=1e-9, return_all=False):
    """The local feedback gain of SOLVED MPC steps: at a strictly complementary solution the QP of mpc_qp_batch is locally affine in x_0,
    u_0(x_0 + dx) = u_0 - K0 dx, and K0 is the first gain of the equality-constrained LQ problem that keeps the active set (csrc/tmpc_mpc_qp_gain.h: one
    backward pass of the constraint-to-go stage of horizon_lqr_batch per instance; no row enters at a penalty weight).

    A, B, H, horizon, phase0, D, d, ndcnt, Pf, penalty, penalty2, J, necnt, terminal as in the mpc_qp_batch call that was solved (q, r, offset, qf,
    terminal_rhs enter only through the solution and are no arguments).  sol: the dict that call returned -- X [nb,ns,N+1,nx], U [nb,ns,N,nu], lam [nb,ns,N,nd]
    with rows, eps with penalty or penalty2 --, validated like guess=.  The class of row (j, i) follows the solver's activity rules, with g = d_i - D_i z_j:
        hard row (penalty inf)                   s = g                                  1 if lam > s, else 0
        pure quadratic (penalty 0, Z > 0)        s = g + lam / Z                        2 if lam > s, else 0
        0 < penalty < inf                        s = g + e, nu = penalty + Z e - lam    0 if not lam > s; else violated (e > nu): 2 if Z > 0, 0 if Z = 0; else 1
        rows beyond ndcnt                                                               0
    0 free: the row drops out; 1 equality: D_i dz_j = 0; 2 quadratic: the stage Hessian gains Z_i D_i' D_i.  The rows of J and the terminal rows always hold.
    active: int32 [nb,ns,N,nd] with entries 0, 1, 2 replaces the rule (the gain at any active set; 2 on a row without penalty2 counts as 0).

    numpy arrays run through the host entry, torch tensors on a GPU through the device entry; both run the same kernel and agree bit for bit, and the numbers
    of an instance do not depend on ns or on the other instances.

    Returns dict: K0 [nb,ns,nu,nx], Pi0 [nb,ns,nx,nx] (projected with Pz_0 = I - Hn0' Hn0: the directions dx with Hn0 dx = 0 are those in which the active set
    can be kept), Hn0 [nb,ns,nx,nx] (cnt0 orthonormal rows, the rest zero), cnt0 int32 [nb,ns], cls int32 [nb,ns,N,nd], nactive int32 [nb,ns,N] (rows of class
    1 or 2 per stage), strict [nb,ns] = min over the complementarity pairs (lam, s) and (e, nu) of |a - b| / max(|a|, |b|) -- near 1: the active set is
    unambiguous; near 0: a weakly active row, the derivative is one-sided and K0 means nothing --, status [nb,ns] (0 done, 2 singular stage system, 3
    non-finite: also an instance whose sol holds NaN, as a failed solve returns, 5 the active set leaves no direction), feas, info [nb,ns,12] as in
    horizon_lqr_batch.  status >= 2: K0, Pi0, strict NaN, cls -1 at the stages that were not finished.  return_all=True adds Kall [nb,ns,N,nu,nx], cntall
    [nb,ns,N], and the open-loop sensitivities dX [nb,ns,N+1,nx,nx], dU [nb,ns,N,nu,nx]: X + dX dx, U + dU dx is the solution at x_0 + dx for dx in the
    feasible subspace while the active set holds.  Not served: sensitivities of the multipliers, the one-sided derivative on a weakly active row.
    ValueError: shapes, dtypes, mixed numpy / torch, a sol that is no dict or lacks an array, active outside 0 .. 2; NotImplementedError: n > 64, shapes
    beyond the 160 KB LDS layout (gain_lds_bytes)."""
    who = 'mpc_qp_gain_batch'
    if not isinstance(sol, dict):
        raise ValueError('{}: sol must be a dict as returned by mpc_qp_batch (X, U, lam, and eps where the problem has it), got {}'.format(who, type(sol).__name__))
    Xs = sol.get('X')
    if Xs is None or not hasattr(Xs, 'shape') or len(Xs.shape) != 4:
        raise ValueError("{}: sol['X'] [nb, ns, horizon + 1, nx] expected, got {} (a call with return_traj=False returns no solution)".format(
            who, None if Xs is None else tuple(getattr(Xs, 'shape', ()))))
    if penalty2 is not None and penalty is None and hasattr(penalty2, 'shape'):      # every row pure quadratic: penalty is taken as 0
        penalty = penalty2.new_zeros(tuple(penalty2.shape)) if lqr._is_torch(penalty2) else np.zeros(penalty2.shape)
    use_torch, nd, N, _, k0 = _validate(who, A, B, H, Xs[:, :, 0], horizon, phase0, D, d, ndcnt, None, Pf, TOL, MAX_ITER, 1, penalty, J, None, necnt, terminal, penalty2)
    if isinstance(rank_tol, bool) or not isinstance(rank_tol, (int, float, np.floating)) or not (0.0 < float(rank_tol) < 1.0):
        raise ValueError('{}: 0 < rank_tol < 1 expected, got {!r}'.format(who, rank_tol))
    nb, p, nx, nu = (int(v) for v in B.shape)
    ns = int(Xs.shape[1])
    ne = 0 if J is None else int(J.shape[2])
    need = gain_lds_bytes(nx, nu, nd, ne)
    if need > LDS_BYTES:
        raise NotImplementedError('{}: nx = {}, nu = {} with room for {} + {} rows per stage and a constraint-to-go needs {} bytes of LDS (limit {})'.format(
            who, nx, nu, ne, nd, need, LDS_BYTES))
    want = [('X', (nb, ns, N + 1, nx), True), ('U', (nb, ns, N, nu), True), ('lam', (nb, ns, N, nd), nd > 0),
            ('eps', (nb, ns, N, nd), nd > 0 and (penalty is not None or penalty2 is not None))]
    got = []
    for key, shape, needed in want:
        x = sol.get(key)
        if not needed:
            got.append(None)
            continue
        if x is None:
            raise ValueError('{}: sol[{!r}] {} expected, got None (a call with return_traj=False returns no solution)'.format(who, key, shape))
        if not hasattr(x, 'shape') or tuple(x.shape) != shape:
            raise ValueError('{}: sol[{!r}] {} expected, got {}'.format(who, key, shape, tuple(x.shape) if hasattr(x, 'shape') else type(x).__name__))
        got.append(x)
    _cl._check_kind(who, [('A', A)] + [('sol[%r]' % k, x) for (k, _, _), x in zip(want, got) if x is not None])
    X, U, Lam, Eps = (lqr._contig(x, use_torch) for x in got)
    if active is not None:
        if nd == 0:
            raise ValueError('{}: active describes the rows of D, which is None'.format(who))
        if not hasattr(active, 'shape') or lqr._is_torch(active) != use_torch:
            raise ValueError('{}: active must be {} like A, B, H'.format(who, 'a torch tensor' if use_torch else 'a numpy array'))
        if tuple(active.shape) != (nb, ns, N, nd) or 'int32' not in str(active.dtype):
            raise ValueError('{}: active int32 {} expected, got {} {}'.format(who, (nb, ns, N, nd), active.dtype, tuple(active.shape)))
        if use_torch and (not active.is_cuda or active.device != A.device):
            raise ValueError('{}: torch tensors must be tensors of one GPU (active: {})'.format(who, active.device))
        lo, hi = int(active.min()), int(active.max())
        if lo < 0 or hi > 2:
            raise ValueError('{}: active in 0 (free), 1 (equality), 2 (quadratic) expected, got {} .. {}'.format(who, lo, hi))
        active = active.contiguous() if use_torch else np.ascontiguousarray(active)
    A, B, H, D, d, Pf, penalty, penalty2, J = (lqr._contig(x, use_torch) for x in (A, B, H, D, d, Pf, penalty, penalty2, J))
    ndcnt, necnt = (None if c is None else (c.contiguous() if use_torch else np.ascontiguousarray(c)) for c in (ndcnt, necnt))
    term, Tx = (0, None) if terminal is None else (1, None) if isinstance(terminal, str) else (2, lqr._contig(terminal, use_torch))
    entry = _lib.mpc_qp_gain_batch_device if use_torch else _lib.mpc_qp_gain_batch_host
    out = entry(A, B, H, Pf, D, ndcnt, d, penalty, penalty2, J, necnt, term, Tx, X, U, Lam, Eps, active, N, k0, float(rank_tol), bool(return_all))
    info, cls = out['info'], out['cls']
    if use_torch:
        import torch
        out.update(status=info[..., 0].to(torch.int32), feas=info[..., 7].clone(), nactive=(cls > 0).sum(dim=-1).to(torch.int32))
    else:
        out.update(status=info[..., 0].astype(np.int32), feas=info[..., 7].copy(), nactive=(cls > 0).sum(axis=-1).astype(np.int32))
    return out


def mpc_step_gain(A, B, Q, R, N, sol, horizon, phase0=0, D=None, d=None, Pf=None, penalty=None, penalty2=None, J=None, terminal=None, active=None,
                  rank_tol=1e-9):
    """The local gain of one solved step of one model in the reference's calling style, beside mpc_step: A, B, Q, R, N, D, d, Pf, penalty, penalty2, J,
    terminal as mpc_step took them; sol a dict with X [horizon+1,nx], U [horizon,nu], lam [horizon,nd] (what mpc_step returned) and eps (its info['eps'])
    with penalties; active int [horizon,nd] or None.  Returns (K0 [nu,nx], info dict: Pi0, Hn0 [cnt0,nx], cnt0, cls, nactive, strict, status, feas).
    RuntimeError when the pass ended with a status != 0."""
    who = 'mpc_step_gain'
    if not isinstance(sol, dict) or sol.get('X') is None:
        raise ValueError('{}: sol must be a dict with X, U, lam (and eps where the problem has it)'.format(who))
    X = _to_array(sol['X']).astype(np.float64)
    As, Bs, Hs, _, kw = _stack_one(who, A, B, Q, R, N, X[0] if X.ndim == 2 else X, D, d, None, Pf, penalty, penalty2)
    kw.pop('q')
    eq = _stack_eq(who, As.shape[1], As.shape[2], As.shape[2] + Bs.shape[3], J, None, terminal)
    kw.update(J=eq['J'], necnt=eq['necnt'], terminal=eq['terminal'])
    s = {k: None if sol.get(k) is None else np.ascontiguousarray(_to_array(sol[k]).astype(np.float64)[None, None]) for k in ('X', 'U', 'lam', 'eps')}
    if s['lam'] is not None and kw['D'] is not None and s['lam'].shape[-1] < kw['D'].shape[2]:
        raise ValueError('{}: sol[\'lam\'] must hold one column per row of D'.format(who))
    act = None if active is None else np.ascontiguousarray(np.asarray(_to_array(active)).astype(np.int32)[None, None])
    res = mpc_qp_gain_batch(As, Bs, Hs, s, horizon, phase0, active=act, rank_tol=rank_tol, **kw)
    st = int(res['status'][0, 0])
    if st != 0:
        raise RuntimeError('{}: the pass ended with status {} ({})'.format(who, st, GAIN_STATUS_NAMES.get(st)))
    c0 = int(res['cnt0'][0, 0])
    return res['K0'][0, 0], dict(Pi0=res['Pi0'][0, 0], Hn0=res['Hn0'][0, 0, :c0], cnt0=c0, cls=res['cls'][0, 0], nactive=res['nactive'][0, 0],
                                 strict=float(res['strict'][0, 0]), status=st, feas=float(res['feas'][0, 0]))


def mpc_gain_equivalence_batch(A, B, H, Hc, X0, horizon, P=None, phase0=0, D=None, d=None, ndcnt=None, q=None, Pf=None, tol=TOL, max_iter=MAX_ITER,
                               penalty=None, penalty2=None, J=None, r=None, necnt=None, terminal=None, rank_tol=1e-9):
    """The feedback-equivalence certificate of the constrained step: the tracking QP on Hc with the terminal weight Pf and the economic QP on H with
    Pf + P[(phase0 + N) mod p] (the convention of horizon_equivalence_batch: the two costs differ by x_0' P x_0 - x_N' P x_N, so they are the same problem)
    are solved from X0 [nb,ns,nx], and the local gains of both sides (mpc_qp_gain_batch) are taken at the active set found on Hc.  Without terminal rows the
    terminal weights must match, so terminal=None needs P (ValueError without it); the other problem keywords as in mpc_qp_batch.

    An instance that fails on either side (an infeasible x_0: status 1 of the solve, NaN solution, status 3 of the pass) returns NaN / False and its statuses;
    the other instances of the batch are not affected.

    Returns dict of numpy arrays [nb,ns]: du0 = max|u0(H) - u0(Hc)| and same_active (the classes of the two solutions agree in every row) -- NaN / False where
    the H side did not converge, e.g. status 2 on an indefinite H --, dK0 = max|K0(H) - K0(Hc)| on the projected gains at the active set of the Hc side,
    dK0_rel = dK0 / max(1, max|K0(Hc)|), subspace_diff = max|Pz_0(H) - Pz_0(Hc)|, strict (of the Hc solution: dK0 means nothing where it is near 0),
    status_qp_H, status_qp_Hc (the solves), status_H, status_Hc (the passes); and K0, K0c, cls as the entries returned them."""
    who = 'mpc_gain_equivalence_batch'
    if terminal is None and P is None:
        raise ValueError('{}: without terminal rows the H side must carry the terminal weight Pf + P[(phase0 + N) mod p] for the two problems to be the '
                         'same: P is needed'.format(who))
    use_torch = _cl._check_kind(who, [('A', A), ('B', B), ('H', H), ('Hc', Hc), ('X0', X0)] + [(nm, x) for nm, x in (('P', P), ('Pf', Pf)) if x is not None])
    if tuple(Hc.shape) != tuple(H.shape):
        raise ValueError('{}: Hc {} expected, got {}'.format(who, tuple(H.shape), tuple(Hc.shape)))
    if P is not None and tuple(P.shape) != tuple(A.shape):
        raise ValueError('{}: P {} expected, got {}'.format(who, tuple(A.shape), tuple(P.shape)))
    PfH = Pf if P is None else (P if Pf is None else Pf + P)
    rows = dict(D=D, d=d, ndcnt=ndcnt, penalty=penalty, J=J, necnt=necnt, terminal=terminal)
    if penalty2 is not None:
        rows['penalty2'] = penalty2
    qp = dict(q=q, tol=tol, max_iter=max_iter, r=r)
    sC = _step(who, A, B, Hc, X0, horizon, phase0, Pf=Pf, **rows, **qp)
    sH = _step(who, A, B, H, X0, horizon, phase0, Pf=PfH, **rows, **qp)
    gC = mpc_qp_gain_batch(A, B, Hc, sC, horizon, phase0, Pf=Pf, rank_tol=rank_tol, **rows)
    # the classes of the Hc side as the override of the H side; an instance that failed there (a NaN solution: status 3, or status 5) left -1 at its unfinished
    # stages: taken as 0 here, that instance ends with status 3 / NaN on its own NaN solution or is masked below, and its neighbours are not touched
    act = None
    if gC['cls'].shape[-1]:
        act = gC['cls'].clamp(min=0) if use_torch else np.maximum(gC['cls'], 0)
    gH = mpc_qp_gain_batch(A, B, H, sC, horizon, phase0, Pf=PfH, rank_tol=rank_tol, active=act, **rows)
    gR = mpc_qp_gain_batch(A, B, H, sH, horizon, phase0, Pf=PfH, rank_tol=rank_tol, **rows)      # the H solution through the rule: its classes
    host = (lambda x: x.cpu().numpy()) if use_torch else (lambda x: np.array(x))
    nb, ns = int(X0.shape[0]), int(X0.shape[1])
    flat = lambda x: host(x).reshape(nb, ns, -1)
    with np.errstate(invalid='ignore'):
        du0 = np.abs(flat(sH['u0']) - flat(sC['u0'])).max(axis=2)
        dK0 = np.abs(flat(gH['K0']) - flat(gC['K0'])).max(axis=2)
        rel = dK0 / np.maximum(1.0, np.abs(flat(gC['K0'])).max(axis=2))
        PzH = np.einsum('bsji,bsjl->bsil', host(gH['Hn0']), host(gH['Hn0'])); PzC = np.einsum('bsji,bsjl->bsil', host(gC['Hn0']), host(gC['Hn0']))
        sd = np.abs(PzH - PzC).reshape(nb, ns, -1).max(axis=2)
    okH = host(sH['status']) == 0
    same = okH & (host(sC['status']) == 0) & (flat(gR['cls']) == flat(gC['cls'])).all(axis=2) & (host(gR['status']) != 3)
    du0 = np.where(okH, du0, np.nan)
    okC = host(gC['status']) == 0                                           # (status 5 on the Hc side: the H side ran at a clamped set, which is no active set)
    dK0, rel, sd = (np.where(okC, x, np.nan) for x in (dK0, rel, sd))
    same = same & okC
    return dict(du0=du0, same_active=same, dK0=dK0, dK0_rel=rel, subspace_diff=sd, strict=host(gC['strict']), status_qp_H=host(sH['status']),
                status_qp_Hc=host(sC['status']), status_H=host(gH['status']), status_Hc=host(gC['status']), K0=gH['K0'], K0c=gC['K0'], cls=gC['cls'])
