"""Closed-loop rollouts of a tuned feedback law on the GPU: the LQ content of the reference's closed_loop_tools.closed_loop_sim.

lqr.py computes the feedback laws a tuned scheme defines (the periodic gains K_k, the first-order law u_0 = -K_0 x_0 of a horizon-N controller from every
phase) and certifies that the H side and the Hc side give the same gains.  This module RUNS a law: ns initial deviations per problem are stepped through

    u_t = -K_k x_t,   x_{t+1} = A_k x_t + B_k u_t,   k = (phase0 + t) mod p,

logging the economic stage cost l_t = 1/2 z_t' H_k z_t, the tracking cost lc_t = 1/2 z_t' Hc_k z_t (z = [x; u]), the residual of the rows max|J_k z_t| and of
a constraint-to-go max|Hn_k x_t| -- one launch for the whole batch (csrc/tmpc_closed_loop.h: a tile of initial states stays in LDS for all steps).

    closed_loop_batch(A, B, K, X0, steps, phase0=0, H=None, Hc=None, J=None, ...)       the rollout (numpy -> host entry, torch GPU tensors -> device entry)
    closed_loop_monodromy_batch(A, B, K, Pz0=None)                                      Phi = (A-BK)_{p-1} ... (A-BK)_0 [Pz0] and its spectral radius, for ANY law
    horizon_closed_loop_batch(A, B, H, horizons, ...)                                   the stabilising-horizon scan: rho of the receding-horizon loop per N
    cost_equivalence_batch(A, B, H, Hc, P, K, X0, steps, ...)                           the trajectory-level certificate of a convexification
    closed_loop_sim(A, B, K, x0, steps, ...)                                            the reference's calling style -> its log {'x', 'u', 'l', 'h'}
    cost_equivalence(A, B, Q, R, N, dHc, P, K, x0, steps, ...)                          the certificate on what `convexify` takes and returns

This is the first-order (LQ) loop: the rows J_k are the ones active at the optimal cycle and stay fixed, the plant is its linearisation.  Changes of the
active set are served by mpc_qp.py (the inequality-constrained MPC in the loop); the nonlinear plant is not simulated.

The certificate: Hc_k = H_k + [A_k B_k]' P_{k+1} [A_k B_k] - diag(P_k, 0) (+ J_k' diag(phi_k) J_k, zero on trajectories that keep the rows), so along ANY
trajectory of the dynamics, whatever the feedback,

    sum_t lc_t - sum_t l_t = 1/2 x_T' P_{(phase0+T) mod p} x_T - 1/2 x_0' P_{phase0} x_0.

No Riccati recursion enters: it tests the supplement and the dynamics, where the gain certificate of lqr.py tests the backward recursion.
Conventions as in lqr.py.  There is no CPU path: the rollout runs in the HIP library or the call raises.
"""
import numpy as np

from . import _lib
from . import lqr
from .convexifier import _to_array

STATUS_NAMES = {0: 'Done', 3: 'NonFinite'}
LDS_BYTES = 160 * 1024


def lds_layout(nx, nu, nr=0):
    """closed_loop_lds of csrc/tmpc_closed_loop.h restated: dict ts (initial states per workgroup; 0: not even one fits), bytes (LDS of a workgroup).
    TS is 64 when two workgroups then share a CU (<= 80 KB each), else the largest power of two that fits the 160 KB; it depends on (nx, nu, nr) alone."""
    nx, nu, nr = int(nx), int(nu), int(nr)
    n = nx + nu
    ldn, ldx = n | 1, nx | 1
    fixed = nx * ldn + nu * ldx + n * ldn + nr * ldn + nx * ldx + 6 * 256 + 64
    budget = LDS_BYTES // 8
    ts = 64
    if fixed + 2 * n * 64 > budget // 2:
        ts = 32
        while ts > 0 and fixed + 2 * n * ts > budget:
            ts >>= 1
    return dict(ts=ts, bytes=8 * (fixed + 2 * n * max(ts, 1)))


def _check_kind(who, named):
    """All arrays numpy fp64 or all torch fp64 tensors of one GPU -> use_torch."""
    use_torch = lqr._is_torch(named[0][1])
    ref = named[0][1]
    for nm, x in named:
        if x is None or not hasattr(x, 'shape') or not hasattr(x, 'dtype'):
            raise ValueError('{}: {} must be an array'.format(who, nm))
        if lqr._is_torch(x) != use_torch:
            raise ValueError('{}: the arrays must be all numpy arrays or all torch tensors ({} differs)'.format(who, nm))
        if use_torch:
            import torch
            if x.dtype != torch.float64 or not x.is_cuda or x.device != ref.device:
                raise ValueError('{}: torch tensors must be float64 tensors of one GPU ({}: {}, {})'.format(who, nm, x.dtype, x.device))
        elif np.asarray(x).dtype != np.float64:
            raise ValueError('{}: fp64 arrays expected ({} has dtype {})'.format(who, nm, np.asarray(x).dtype))
    return use_torch


def _validate(who, A, B, K, X0, like_H=(), like_A=()):
    """Shapes and dtypes of a rollout, before the library is loaded.  like_H / like_A: (name, array-or-None) further arrays of the shape [nb,p,n,n] /
    [nb,p,nx,nx].  Returns (use_torch, nb, p, nx, nu, ns)."""
    named = [('A', A), ('B', B), ('K', K), ('X0', X0)] + [(nm, x) for nm, x in tuple(like_H) + tuple(like_A) if x is not None]
    use_torch = _check_kind(who, named)
    if len(A.shape) != 4 or A.shape[2] != A.shape[3]:
        raise ValueError('{}: A [nb, p, nx, nx] expected, got {}'.format(who, tuple(A.shape)))
    nb, p, nx, _ = (int(v) for v in A.shape)
    if len(B.shape) != 4 or tuple(B.shape[:3]) != (nb, p, nx):
        raise ValueError('{}: B [nb, p, nx, nu] = [{}, {}, {}, nu] expected, got {}'.format(who, nb, p, nx, tuple(B.shape)))
    nu = int(B.shape[3])
    if nb < 1 or p < 1 or nx < 1 or nu < 1:
        raise ValueError('{}: nb, p, nx, nu >= 1 expected, got nb = {}, p = {}, nx = {}, nu = {}'.format(who, nb, p, nx, nu))
    if tuple(K.shape) != (nb, p, nu, nx):
        raise ValueError('{}: K [nb, p, nu, nx] = {} expected, got {}'.format(who, (nb, p, nu, nx), tuple(K.shape)))
    if len(X0.shape) != 3 or int(X0.shape[0]) != nb or int(X0.shape[2]) != nx:
        raise ValueError('{}: X0 [nb, ns, nx] = [{}, ns, {}] expected, got {}'.format(who, nb, nx, tuple(X0.shape)))
    ns = int(X0.shape[1])
    if ns < 1:
        raise ValueError('{}: ns >= 1 initial states expected, got X0 {}'.format(who, tuple(X0.shape)))
    n = nx + nu
    for group, want in ((like_H, (nb, p, n, n)), (like_A, (nb, p, nx, nx))):
        for nm, x in group:
            if x is not None and tuple(x.shape) != want:
                raise ValueError('{}: {} {} expected, got {}'.format(who, nm, want, tuple(x.shape)))
    return use_torch, nb, p, nx, nu, ns


def _validate_steps(who, steps, phase0, p):
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or int(steps) < 1:
        raise ValueError('{}: steps must be an int >= 1, got {!r}'.format(who, steps))
    if isinstance(phase0, bool) or not isinstance(phase0, (int, np.integer)) or not (0 <= int(phase0) < p):
        raise ValueError('{}: phase0 must be an int in 0 .. p - 1 = {}, got {!r}'.format(who, p - 1, phase0))
    return int(steps), int(phase0)


def _refuse_beyond_layout(who, nx, nu, nr):
    if nx + nu > 64:
        raise NotImplementedError('{}: the closed-loop rollout handles stage blocks up to nx + nu = 64 (got {})'.format(who, nx + nu))
    lay = lds_layout(nx, nu, nr)
    if lay['ts'] < 1 or lay['bytes'] > LDS_BYTES:
        raise NotImplementedError('{}: nx = {}, nu = {} with room for {} rows per stage needs {} bytes of LDS for a single state (limit {})'.format(
            who, nx, nu, nr, lay['bytes'], LDS_BYTES))


def closed_loop_batch(A, B, K, X0, steps, phase0=0, H=None, Hc=None, J=None, ncnt=None, ng=None, Hn=None, return_traj=True):
    """Rollouts of u = -K_k x on nb p-periodic models: A [nb,p,nx,nx], B [nb,p,nx,nu], K [nb,p,nu,nx] (any phase-indexed law: the K of periodic_lqr_batch, the
    K0 of horizon_lqr_batch over all phases), X0 [nb,ns,nx], fp64, n = nx + nu <= 64; `steps` steps t = 0 .. steps-1 at the stages k = (phase0 + t) mod p.
    Optional: H, Hc [nb,p,n,n] (stage costs l, lc), J [nb,p,nr,n] with ncnt [nb,p] int32 and ng as in periodic_lqr_batch (rowres_t = max|J_k z_t| over the
    first r_k = ng + ncnt_k rows), Hn [nb,p,nx,nx] (subres_t = max|Hn_k x_t| over all rows; the Hn of the constraint-to-go entries, rows beyond c_k zero).

    numpy arrays run through the host entry; torch tensors on a GPU through the device entry (torch tensors out, the inputs are not copied).  Both run the
    same kernel and agree bit for bit; the numbers of a state do not depend on ns or on the other states of the call.

    Returns dict: X [nb,ns,steps+1,nx], U [nb,ns,steps,nu] (None with return_traj=False), l, lc, rowres, subres [nb,ns,steps] (None without their input),
    XT [nb,ns,nx] = x_T, L, Lc [nb,ns] (sum_t l_t, sum_t lc_t, added in the order of t inside the kernel; None without the cost), status [nb,ns] int32 (0 done,
    3 non-finite: a non-finite value in an input or overflow during the rollout; there are no other statuses), steps [nb,ns] int32 (steps finished), xmax
    [nb,ns] = max_t max|x_t|, info [nb,ns,4].  A state with status 3 stopped at step t = steps[b,s]: its U, l, lc, rowres, subres from t on, its X from t + 1
    on, XT, L, Lc are NaN; the other states are not affected.  X, U and the per-step scalars are permuted views of time-major arrays (the kernel's stores of one
    step are contiguous).  ValueError: shapes, dtypes, mixed numpy / torch, steps < 1, phase0 outside 0 .. p-1, ns < 1, ncnt / ng without J;
    NotImplementedError: n > 64, (nx, nu, nr) beyond the 160 KB LDS layout (lds_layout), more than 65535 tiles of states."""
    who = 'closed_loop_batch'
    use_torch, nb, p, nx, nu, ns = _validate(who, A, B, K, X0, (('H', H), ('Hc', Hc)), (('Hn', Hn),))
    T, k0 = _validate_steps(who, steps, phase0, p)
    if J is None and (ncnt is not None or ng is not None):
        raise ValueError('{}: ncnt / ng describe the rows of J, which is None'.format(who))
    nr, ng_ = 0, 0
    if J is not None:
        nr, ng_ = lqr._relabel(lqr._validate_rows, who, J, ncnt, ng, use_torch, A, nb, p, nx + nu)
        if ng_ > nr:
            raise ValueError('{}: ng <= J.shape[2] = {} expected, got {}'.format(who, nr, ng_))
    _refuse_beyond_layout(who, nx, nu, nr)
    A, B, K, X0, H, Hc, J, Hn = (lqr._contig(x, use_torch) for x in (A, B, K, X0, H, Hc, J, Hn))
    if ncnt is not None:
        ncnt = ncnt.contiguous() if use_torch else np.ascontiguousarray(ncnt)
    entry = _lib.closed_loop_batch_device if use_torch else _lib.closed_loop_batch_host
    out = entry(A, B, K, X0, H, Hc, J if nr else None, ncnt if nr else None, ng_, Hn, T, k0, bool(return_traj))
    info, sums = out['info'], out.pop('sums')
    if use_torch:
        import torch
        status = info[..., 0].to(torch.int32); done = info[..., 1].to(torch.int32); xmax = info[..., 2].clone()
    else:
        status = info[..., 0].astype(np.int32); done = info[..., 1].astype(np.int32); xmax = info[..., 2].copy()
    out.update(L=sums[..., 0] if H is not None else None, Lc=sums[..., 1] if Hc is not None else None, status=status, steps=done, xmax=xmax)
    return out


def _eye_like(ref, nb, nx, use_torch):
    if use_torch:
        import torch
        return torch.eye(nx, dtype=torch.float64, device=ref.device).expand(nb, nx, nx).contiguous()
    return np.ascontiguousarray(np.broadcast_to(np.eye(nx), (nb, nx, nx)))


def _t(x, use_torch):
    """Transpose of the last two axes, contiguous."""
    return x.transpose(-1, -2).contiguous() if use_torch else np.ascontiguousarray(np.swapaxes(x, -1, -2))


def _host(x):
    return x.cpu().numpy() if lqr._is_torch(x) else np.asarray(x)


def closed_loop_monodromy_batch(A, B, K, Pz0=None):
    """The closed-loop monodromy of ANY phase-indexed law K [nb,p,nu,nx]: the rollout of X0 = I (or of the columns of Pz0 [nb,nx,nx]) for p steps from phase 0,
    Phi = (A-BK)_{p-1} ... (A-BK)_0 [Pz0].  For the gains of the constraint-to-go and horizon entries, which hold on the feasible subspace only,
    Pz0 = I - Hn_0' Hn_0.  Returns dict Phi [nb,nx,nx] (NaN where the rollout was not finite), rho [nb] (numpy: its spectral radius, NaN likewise),
    status [nb] int32 (numpy: the worst status of the nx rollouts)."""
    who = 'closed_loop_monodromy_batch'
    if not hasattr(A, 'shape') or len(A.shape) != 4 or A.shape[2] != A.shape[3] or min(int(v) for v in A.shape) < 1:
        raise ValueError('{}: A [nb, p, nx, nx] expected, got {}'.format(who, tuple(getattr(A, 'shape', ()))))
    nb, p, nx = int(A.shape[0]), int(A.shape[1]), int(A.shape[2])
    use_torch = lqr._is_torch(A)
    if Pz0 is None:
        X0 = _eye_like(A, nb, nx, use_torch)
    else:
        _check_kind(who, [('A', A), ('Pz0', Pz0)])
        if tuple(Pz0.shape) != (nb, nx, nx):
            raise ValueError('{}: Pz0 [nb, nx, nx] = {} expected, got {}'.format(who, (nb, nx, nx), tuple(Pz0.shape)))
        X0 = _t(Pz0, use_torch)                                               # state j of the rollout: column j of Pz0
    try:
        r = closed_loop_batch(A, B, K, X0, p, return_traj=False)
    except ValueError as e:
        raise ValueError(str(e).replace('closed_loop_batch', who)) from None
    Phi = _t(r['XT'], use_torch)                                              # XT[b, j] = Phi X0[b, j]: the columns of Phi
    return dict(Phi=Phi, rho=lqr._rho(_host(Phi)), status=_host(r['status']).max(axis=1).astype(np.int32))


def horizon_closed_loop_batch(A, B, H, horizons, terminal='cost', Pf=None, J=None, ncnt=None, ng=None, rank_tol=1e-9):
    """The stabilising-horizon scan: for each N in `horizons` the first-order law of the horizon-N controller from all p phases (horizon_lqr_batch, arguments
    as there) is put in the loop, x_{k+1} = (A_k - B_k K_0(k)) x_k, and the monodromy of that receding-horizon loop is taken on the feasible subspace of
    phase 0 (Pz0 = I - Hn0(0)' Hn0(0)).  Returns dict of numpy arrays: rho [nb,nh] (spectral radius; NaN where a pass failed), status [nb,nh] (the worst
    status of horizon_lqr_batch over the phases: 0, 2, 3 or 5), subres [nb,nh] = max_k max|Hn0(k+1) x_{k+1}| along the period for the columns of Pz0 (whether
    the receding-horizon law keeps the state inside the next phase's feasible set; NaN where a pass failed), horizons; and Phi [nb,nh,nx,nx] in the kind of
    the inputs.  Which horizon is long enough: rho < 1, and rho close to the periodic value of periodic_lqr_batch."""
    who = 'horizon_closed_loop_batch'
    hz = np.asarray(horizons)
    if hz.ndim != 1 or hz.size < 1 or hz.dtype.kind not in 'iu' or (hz < 1).any():
        raise ValueError('{}: horizons must be a non-empty list of ints >= 1, got {!r}'.format(who, horizons))
    rho, status, subres, Phis = [], [], [], []
    for N in hz.tolist():
        try:
            h = lqr.horizon_lqr_batch(A, B, H, int(N), terminal=terminal, Pf=Pf, J=J, ncnt=ncnt, ng=ng, rank_tol=rank_tol)
        except ValueError as e:
            raise ValueError(str(e).replace('horizon_lqr_batch', who)) from None
        use_torch = lqr._is_torch(A)
        nb, p, nx = int(A.shape[0]), int(A.shape[1]), int(A.shape[2])
        Hn0 = h['Hn0']
        Pz0 = _eye_like(A, nb, nx, use_torch) - (_t(Hn0[:, 0], use_torch) @ Hn0[:, 0])
        r = closed_loop_batch(A, B, h['K0'], _t(Pz0, use_torch), p, Hn=Hn0, return_traj=False)
        Phi = _t(r['XT'], use_torch)
        wrap = (Hn0[:, 0] @ Phi)                                              # Hn0(0) x_p: the period closes on the feasible set of phase 0
        sub = _host(r['subres'])[:, :, 1:].reshape(nb, -1)
        sub = np.concatenate([sub, np.abs(_host(wrap)).reshape(nb, -1)], axis=1)
        st = _host(h['status']).max(axis=1)
        bad = (st != 0) | (_host(r['status']).max(axis=1) != 0)
        with np.errstate(invalid='ignore'):
            sub = np.where(bad, np.nan, sub.max(axis=1))
        rh = lqr._rho(_host(Phi)); rh[bad] = np.nan
        rho.append(rh); status.append(st.astype(np.int32)); subres.append(sub); Phis.append(Phi)
    if lqr._is_torch(A):
        import torch
        Phi = torch.stack(Phis, dim=1)
    else:
        Phi = np.stack(Phis, axis=1)
    return dict(rho=np.stack(rho, axis=1), status=np.stack(status, axis=1), subres=np.stack(subres, axis=1), Phi=Phi, horizons=hz.astype(np.int64))


def cost_equivalence_batch(A, B, H, Hc, P, K, X0, steps, phase0=0, J=None, ncnt=None, ng=None):
    """The trajectory-level certificate of a convexification: ONE rollout of u = -K_k x (any K) with both costs, and the telescoping identity

        Lc - L = 1/2 x_T' P_{(phase0+T) mod p} x_T - 1/2 x_0' P_{phase0} x_0

    for Hc_k = H_k + [A_k B_k]' P_{k+1} [A_k B_k] - diag(P_k, 0).  With rows carrying multipliers Hc also holds J_k' diag(phi_k) J_k, which vanishes only on
    trajectories that keep J_k z_t = 0: pass J (ncnt, ng) and read rowres, the identity holds up to that residual.  Returns dict of numpy arrays [nb,ns]:
    defect = |Lc - L - (1/2 x_T' P x_T - 1/2 x_0' P x_0)|, defect_rel = defect / max(tiny, sum_t (|l_t| + |lc_t|) + |1/2 x_0' P x_0| + |1/2 x_T' P x_T|),
    rowres = max_t rowres_t (0 without J), L, Lc, status.  It is independent of any Riccati recursion: it tests the supplement and the dynamics."""
    who = 'cost_equivalence_batch'
    for nm, x in (('H', H), ('Hc', Hc), ('P', P)):
        if x is None:
            raise ValueError('{}: {} must be an array'.format(who, nm))
    use_torch, nb, p, nx, nu, ns = _validate(who, A, B, K, X0, (('H', H), ('Hc', Hc)), (('P', P),))
    T, k0 = _validate_steps(who, steps, phase0, p)
    try:
        r = closed_loop_batch(A, B, K, X0, T, k0, H=H, Hc=Hc, J=J, ncnt=ncnt, ng=ng, return_traj=False)
    except ValueError as e:
        raise ValueError(str(e).replace('closed_loop_batch', who)) from None
    if use_torch:
        import torch
        quad = lambda Pk, x: 0.5 * torch.einsum('bsi,bij,bsj->bs', x, Pk, x)
        scale = r['l'].abs().sum(dim=2) + r['lc'].abs().sum(dim=2)
    else:
        quad = lambda Pk, x: 0.5 * np.einsum('bsi,bij,bsj->bs', x, Pk, x)
        scale = np.abs(r['l']).sum(axis=2) + np.abs(r['lc']).sum(axis=2)
    v0 = _host(quad(P[:, k0], X0)); vT = _host(quad(P[:, (k0 + T) % p], r['XT']))
    L, Lc, scale = _host(r['L']), _host(r['Lc']), _host(scale)
    with np.errstate(invalid='ignore'):
        defect = np.abs(Lc - L - (vT - v0))
        rel = defect / np.maximum(np.finfo(np.float64).tiny, scale + np.abs(v0) + np.abs(vT))
    rowres = np.zeros((nb, ns)) if r['rowres'] is None else _host(r['rowres'].max(dim=2).values if use_torch else r['rowres'].max(axis=2))
    return dict(defect=defect, defect_rel=rel, rowres=rowres, L=L, Lc=Lc, status=_host(r['status']))


def _stack_gains(K, p, nu, nx, who):
    Ks = [_to_array(k) for k in K] if isinstance(K, (list, tuple)) else [_to_array(K)] * p
    if len(Ks) != p or any(k.shape != (nu, nx) for k in Ks):
        raise ValueError('{}: K must be one (nu, nx) matrix or a list of p = {} of them'.format(who, p))
    return np.ascontiguousarray(np.stack(Ks)[None], dtype=np.float64)


def _zero_costs(A, B, Q, R, N):
    """Q, R, N may be left out in closed_loop_sim (no cost log): zeros of the right shapes, single or per stage like A."""
    As = A if isinstance(A, (list, tuple)) else [A]
    Bs = B if isinstance(B, (list, tuple)) else [B]
    nx, nu = _to_array(As[0]).shape[0], _to_array(Bs[0]).shape[1]
    z = lambda X, sh: [np.zeros(sh) for _ in As] if X is None and isinstance(A, (list, tuple)) else (np.zeros(sh) if X is None else X)
    return z(Q, (nx, nx)), z(R, (nu, nu)), z(N, (nx, nu))


def closed_loop_sim(A, B, K, x0, steps, phase0=0, Q=None, R=None, N=None, dHc=None, G=None, C=None):
    """One model in the reference's calling style (closed_loop_tools.closed_loop_sim with the LQ controller u = -K_k x in the loop and the linear plant):
    A, B single matrices (p = 1) or lists of length p, K one gain or a list of p (as periodic_lqr returns them), x0 the initial deviation, Q, R, N the
    economic stage cost (left out: zero), dHc the supplements of `convexify` (then the log gains 'lc', the cost on Hc = H + dHc), G, C the rows as `convexify`
    takes them.  Returns the reference's log: {'x': steps + 1 states, 'u': steps inputs, 'l': steps stage costs, 'h': steps arrays J_k [x_t; u_t], the
    constraint function along the way (empty without rows)}.  RuntimeError when the rollout was not finite."""
    who = 'closed_loop_sim'
    costs = Q is not None or R is not None or N is not None
    Q, R, N = _zero_costs(A, B, Q, R, N)
    try:
        As, Bs, Hs, rows = lqr._stack_stages(A, B, Q, R, N, G, C)
    except ValueError as e:
        raise ValueError(str(e).replace('periodic_lqr', who)) from None
    p, nx, nu = As.shape[1], As.shape[2], Bs.shape[3]
    Ks = _stack_gains(K, p, nu, nx, who)
    x = _to_array(x0).astype(np.float64).reshape(-1)
    if x.shape != (nx,):
        raise ValueError('{}: x0 must hold nx = {} entries, got {}'.format(who, nx, _to_array(x0).shape))
    Hcs = None
    if dHc is not None:
        dH = np.stack([_to_array(d) for d in (dHc if isinstance(dHc, (list, tuple)) else [dHc])])[None]
        if dH.shape != Hs.shape:
            raise ValueError('{}: dHc must hold p matrices (nx+nu, nx+nu), got {}'.format(who, dH.shape[1:]))
        Hcs = Hs + dH
    r = closed_loop_batch(As, Bs, Ks, np.ascontiguousarray(x[None, None]), steps, phase0, H=Hs, Hc=Hcs, **rows)
    if int(r['status'][0, 0]) != 0:
        raise RuntimeError('{}: the rollout met a non-finite value at step {} of {}'.format(who, int(r['steps'][0, 0]), int(steps)))
    T = int(steps)
    X, U = r['X'][0, 0], r['U'][0, 0]
    log = {'x': [X[t].copy() for t in range(T + 1)], 'u': [U[t].copy() for t in range(T)], 'l': [float(v) for v in r['l'][0, 0]] if costs else [0.0] * T, 'h': []}
    for t in range(T):
        k = (int(phase0) + t) % p
        if rows:
            rk = int(rows['ng']) + (int(rows['ncnt'][0, k]) if 'ncnt' in rows else 0)
            log['h'].append(rows['J'][0, k, :rk] @ np.concatenate([X[t], U[t]]))
        else:
            log['h'].append(np.zeros(0))
    if Hcs is not None:
        log['lc'] = [float(v) for v in r['lc'][0, 0]]
    return log


def cost_equivalence(A, B, Q, R, N, dHc, P, K, x0, steps, phase0=0, G=None, C=None):
    """cost_equivalence_batch for one model in the calling style of `convexify`: dHc is its first return value (list of p supplements), P its second (list of p
    matrices), G, C the rows it was called with, K one gain or a list of p, x0 one initial deviation or an array [ns, nx] of them.  Returns the dict of the
    batched call with one entry per initial state (arrays [ns]; ints for status)."""
    who = 'cost_equivalence'
    try:
        As, Bs, Hs, rows = lqr._stack_stages(A, B, Q, R, N, G, C)
    except ValueError as e:
        raise ValueError(str(e).replace('periodic_lqr', who)) from None
    p, nx, nu = As.shape[1], As.shape[2], Bs.shape[3]
    dH = np.stack([_to_array(d) for d in (dHc if isinstance(dHc, (list, tuple)) else [dHc])])[None]
    if dH.shape != Hs.shape:
        raise ValueError('{}: dHc must hold p matrices (nx+nu, nx+nu), got {}'.format(who, dH.shape[1:]))
    Ps = lqr._stack_weights(P, p, nx, 'P')
    if Ps is None:
        raise ValueError('{}: P must be one (nx, nx) matrix or a list of p = {} of them'.format(who, p))
    X0 = np.ascontiguousarray(np.atleast_2d(_to_array(x0).astype(np.float64)))
    if X0.ndim != 2 or X0.shape[1] != nx:
        X0 = X0.reshape(1, -1)
    r = cost_equivalence_batch(As, Bs, Hs, Hs + dH, Ps, _stack_gains(K, p, nu, nx, who), np.ascontiguousarray(X0[None]), steps, phase0, **rows)
    return {k: v[0] for k, v in r.items()}
