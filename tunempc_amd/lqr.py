"""Periodic LQR gains on the GPU and the feedback-equivalence certificate of a convexification.

The convexifier promises (reference convexifier.py:44-45) that the LQR problem on the convexified Hessian H + dH has the same feedback
law as the one on the indefinite H; the reference checks it once, at p = 1, with two `dare` calls (examples/convex_lqr.py:52-58).  This
module computes the gains K_k of a p-periodic problem by backward Riccati sweeps (one launch per batch, csrc/tmpc_lqr.h) and measures
that sentence on any batch:

    periodic_lqr_batch(A, B, H, Pi0=None, tol=1e-13, max_sweeps=5000)     batched arrays (numpy -> host entry, torch GPU tensors -> device entry)
    periodic_lqr(A, B, Q, R, N)                                           the reference's calling style -> (K_list, Pi_list, rho)
    feedback_equivalence_batch(A, B, H, Hc, P=None)                       max |K(H) - K(Hc)| per problem, both closed-loop spectral radii
    feedback_equivalence(A, B, Q, R, N, dHc)                              the same on what `convexify` takes and returns

For the models with rows (Step 1 with G, Steps 2 / 3 with C) the equivalence holds for the LQ problems that keep J_k [x_k; u_k] = 0, J_k = [G_k; C_k]:
every call takes the rows (J=, ncnt=, ng= in the layout of convexify_step2_batch's library call; G=, C= as `convexify` takes them) and then runs the
recursion with the rows held as equalities (csrc/tmpc_lqr_rows.h).  Without them the calls are the plain ones, bit for bit.

That recursion serves r_k <= nu rows with an input part of full row rank.  state_rows=True (with rank_tol=) selects the constraint-to-go recursion
(csrc/tmpc_lqr_ctg.h) for everything else: more rows than inputs, rows on the state alone, dependent rows.  What the rows say about x_k alone is carried
backwards as Hn_k x_k = 0; gains and cost-to-go are returned projected on the feasible subspace, Pz_k = I - Hn_k' Hn_k, where they are unique, and the
certificate compares the projected gains and the subspaces of the two sides.  An empty feasible subspace ends a problem with status 5.

The controllers a user builds are finite-horizon ones (reference tuner.py:162, pmpc.py:162-281): horizon N, started at whatever phase the plant is in, ended
by a terminal weight or by x_N = 0.  Their first-order feedback u_0 = -K_0 x_0 is not the periodic gain unless N is long, and the statement to certify is that
the tracking MPC on Hc and the economic MPC on H give the same K_0 at every phase (the LQ content of closed_loop_tools.check_equivalence):

    horizon_lqr_batch(A, B, H, horizon, terminal='constraint' | 'cost', Pf=None, phases=None, ...)      K_0 of every (problem, starting phase), one backward pass each
    horizon_lqr(A, B, Q, R, N, horizon, ...)                                                            the reference's calling style
    horizon_equivalence_batch(A, B, H, Hc, horizon, P=None, ...)                                        max |K_0(H) - K_0(Hc)| per (problem, phase)
    horizon_equivalence(A, B, Q, R, N, dHc, horizon, ...)                                               the same on what `convexify` takes and returns

(csrc/tmpc_lqr_horizon.h: the stage of the constraint-to-go recursion, so any rows are served; a terminal constraint is that recursion started from Hn_N = I.)

Conventions: stage cost 1/2 [x;u]' H_k [x;u] with H_k = [[Q_k, N_k], [N_k', R_k]] (x block first, the layout of convexify_batch),
x_{k+1} = A_k x_k + B_k u_k, and u = -K_k x: the sign of scipy.linalg.solve_discrete_are / control.dare.
There is no CPU path: the recursion runs in the HIP library or the call raises.
"""
import numpy as np

from . import _lib
from . import preprocessing
from .convexifier import _to_array, pack_rows

STATUS_NAMES = {0: 'Converged', 1: 'MaxSweeps', 2: 'SingularS', 3: 'NonFinite', 4: 'RowsExceedInputs', 5: 'NoFeasibleSubspace'}


def _is_torch(x):
    return type(x).__module__.split('.')[0] == 'torch'


def _validate(A, B, H, extra=()):
    """Shapes and dtypes of a batch, before any device call.  extra: (name, array-or-None, 'A' | 'H') further arrays of the shape of A or of H.
    Returns (use_torch, nb, p, nx, mb)."""
    named = [('A', A), ('B', B), ('H', H)] + [(nm, x) for nm, x, _ in extra if x is not None]
    use_torch = _is_torch(A)
    for nm, x in named:
        if _is_torch(x) != use_torch:
            raise ValueError('periodic_lqr_batch: A, B, H (and Pi0 / Hc / P) must be all numpy arrays or all torch tensors ({} differs)'.format(nm))
        if x is None or not hasattr(x, 'shape') or not hasattr(x, 'dtype'):
            raise ValueError('periodic_lqr_batch: {} must be an array'.format(nm))
        if use_torch:
            import torch
            if x.dtype != torch.float64 or not x.is_cuda or x.device != A.device:
                raise ValueError('periodic_lqr_batch: torch tensors must be float64 tensors of one GPU ({}: {}, {})'.format(nm, x.dtype, x.device))
        elif np.asarray(x).dtype != np.float64:
            raise ValueError('periodic_lqr_batch: fp64 arrays expected ({} has dtype {})'.format(nm, np.asarray(x).dtype))
    if len(A.shape) != 4 or A.shape[2] != A.shape[3]:
        raise ValueError('periodic_lqr_batch: A [nb, p, nx, nx] expected, got {}'.format(tuple(A.shape)))
    nb, p, nx, _ = (int(v) for v in A.shape)
    if len(B.shape) != 4 or tuple(B.shape[:3]) != (nb, p, nx):
        raise ValueError('periodic_lqr_batch: B [nb, p, nx, nu] = [{}, {}, {}, nu] expected, got {}'.format(nb, p, nx, tuple(B.shape)))
    mb = int(B.shape[3])
    if nb < 1 or p < 1 or nx < 1 or mb < 1:
        raise ValueError('periodic_lqr_batch: nb, p, nx, nu >= 1 expected, got nb = {}, p = {}, nx = {}, nu = {}'.format(nb, p, nx, mb))
    n = nx + mb
    if tuple(H.shape) != (nb, p, n, n):
        raise ValueError('periodic_lqr_batch: H [nb, p, nx + nu, nx + nu] = {} expected, got {}'.format((nb, p, n, n), tuple(H.shape)))
    for nm, x, like in extra:
        want = (nb, p, nx, nx) if like == 'A' else (nb, p, n, n)
        if x is not None and tuple(x.shape) != want:
            raise ValueError('periodic_lqr_batch: {} {} expected, got {}'.format(nm, want, tuple(x.shape)))
    return use_torch, nb, p, nx, mb


def _validate_rows(J, ncnt, ng, use_torch, ref, nb, p, n):
    """Shapes, dtypes and ranges of the rows, before any device call -> (nr, ng).  J [nb,p,nr,n] fp64; ncnt [nb,p] int32 or None (ng rows at every
    stage); ng None: nr without ncnt, 0 with it.  ng > nr is left to the library (its message)."""
    if ng is not None and (isinstance(ng, bool) or not isinstance(ng, (int, np.integer))):
        raise ValueError('periodic_lqr_batch: ng must be an int, got {!r}'.format(ng))
    for nm, x in (('J', J), ('ncnt', ncnt)):
        if x is None:
            continue
        if not hasattr(x, 'shape') or not hasattr(x, 'dtype') or _is_torch(x) != use_torch:
            raise ValueError('periodic_lqr_batch: {} must be {} like A, B, H'.format(nm, 'a torch tensor' if use_torch else 'a numpy array'))
        if use_torch and (not x.is_cuda or x.device != ref.device):
            raise ValueError('periodic_lqr_batch: torch tensors must be tensors of one GPU ({}: {})'.format(nm, x.device))
    import_torch = None
    if use_torch:
        import torch as import_torch
    if J.dtype != (import_torch.float64 if use_torch else np.float64):
        raise ValueError('periodic_lqr_batch: fp64 arrays expected (J has dtype {})'.format(J.dtype))
    if len(J.shape) != 4 or (int(J.shape[0]), int(J.shape[1]), int(J.shape[3])) != (nb, p, n):
        raise ValueError('periodic_lqr_batch: J [nb, p, nr, nx + nu] = [{}, {}, nr, {}] expected, got {}'.format(nb, p, n, tuple(J.shape)))
    nr = int(J.shape[2])
    if ng is None:
        ng = nr if ncnt is None else 0
    ng = int(ng)
    if ng < 0:
        raise ValueError('periodic_lqr_batch: ng >= 0 expected, got {}'.format(ng))
    if ncnt is not None:
        if ncnt.dtype != (import_torch.int32 if use_torch else np.int32):
            raise ValueError('periodic_lqr_batch: ncnt must be int32 (got dtype {})'.format(ncnt.dtype))
        if tuple(ncnt.shape) != (nb, p):
            raise ValueError('periodic_lqr_batch: ncnt [nb, p] = {} expected, got {}'.format((nb, p), tuple(ncnt.shape)))
        if ng <= nr and (bool((ncnt < 0).any()) or bool((ncnt > nr - ng).any())):
            raise ValueError('periodic_lqr_batch: 0 <= ncnt <= J.shape[2] - ng = {} expected'.format(nr - ng))
    return nr, ng


def _contig(x, use_torch):
    if x is None:
        return None
    return x.contiguous() if use_torch else np.ascontiguousarray(x, dtype=np.float64)


def _rho(Phi):
    """Spectral radius of each closed-loop monodromy (host, numpy.linalg.eigvals: nb small matrices); nan where Phi is not finite."""
    Phi = np.asarray(Phi)
    out = np.full(Phi.shape[0], np.nan)
    ok = np.isfinite(Phi).all(axis=(1, 2))
    if ok.any():
        out[ok] = np.abs(np.linalg.eigvals(Phi[ok])).max(axis=1)
    return out


def _subspace_diff(nH, nC, use_torch):
    """max_k max|Pz_k(H side) - Pz_k(Hc side)| per problem from the two Hn [nb,p,nx,nx] (Pz = I - Hn' Hn), computed where the arrays live -> numpy [nb]."""
    if use_torch:
        import torch
        d = (torch.einsum('bkji,bkjl->bkil', nH, nH) - torch.einsum('bkji,bkjl->bkil', nC, nC)).abs()
        return d.reshape(d.shape[0], -1).max(dim=1).values.cpu().numpy()
    d = np.abs(np.einsum('bkji,bkjl->bkil', nH, nH) - np.einsum('bkji,bkjl->bkil', nC, nC))
    return d.reshape(d.shape[0], -1).max(axis=1)


def periodic_lqr_batch(A, B, H, Pi0=None, tol=1e-13, max_sweeps=5000, J=None, ncnt=None, ng=None, state_rows=False, rank_tol=1e-9):
    """Gains of nb p-periodic LQ problems.  A [nb,p,nx,nx], B [nb,p,nx,nu], H [nb,p,n,n] (n = nx + nu <= 64), fp64; per stage, indices mod p,

        E = [A_k B_k],  Hb = H_k + E' Pi_{k+1} E,  S = Hb_uu,  M = Hb_ux,  K_k = S^-1 M  (u = -K_k x),  Pi_k = sym(Hb_xx - M' K_k),

    swept k = p-1 ... 0 from Pi = Pi0 [nb,p,nx,nx] (None: zero) until max_k max|dPi_k| / max(1, max|Pi_k|) <= tol or max_sweeps sweeps.
    S is solved by elimination with row pivoting: it need not be positive definite (from zero it usually is not for an indefinite H).

    numpy arrays run through the host entry; torch tensors on a GPU through the device entry (torch tensors out, A / B / H are not copied).
    Returns dict: K [nb,p,nu,nx], Pi [nb,p,nx,nx], Phi [nb,nx,nx] (closed-loop monodromy (A-BK)_{p-1} ... (A-BK)_0), rho [nb] (numpy: its
    spectral radius, nan where Phi is not finite), status [nb] (0 converged, 1 max_sweeps reached, 2 singular S, 3 non-finite iterate),
    sweeps [nb], info [nb,8] (status, sweeps, last relative change, smallest / largest |pivot| of S in the last sweep, 1.0 if S was shown
    positive definite at every stage of the last sweep, the same over every sweep of the call, reserved).  ValueError: shapes / dtypes; NotImplementedError: n > 64.

    With rows -- J [nb,p,nr,n] fp64, ncnt [nb,p] int32 (None: ng rows at every stage), ng (None: nr without ncnt, 0 with it); stage k holds
    J_k [x_k; u_k] = 0 for its first r_k = ng + ncnt_k rows J_k = [Jx | Ju], the layout of the Step 2 / Step 3 library calls -- the stage solve is

        [[S, Ju'], [Ju, 0]] [K_k; Lam_k] = [M; Jx],   Pi_k = sym(Hb_xx - [M; Jx]' [K_k; Lam_k]),   so that Jx - Ju K_k = 0,

    and the dict gains Lam [nb,p,nr,nx] (zero beyond r_k) and feas [nb] = info[:, 7] = max_k max|Jx - Ju K_k|; info[:, 5:7] then read 1.0 when every
    stage problem was shown convex (S positive definite and Ju of full row rank).  Served: r_k <= nu with Ju of full row rank.  status 4
    (RowsExceedInputs): r_k > nu at some stage -- sweeps 0, K and Lam zero, Pi = Pi0, Phi NaN; status 2 also covers a rank-deficient Ju.  Rows that
    constrain the state alone (Ju = 0) would need a constraint-to-go recursion: not provided, they end with status 2.  NotImplementedError also for
    (nx, nu, nr) beyond the 160 KB of LDS (n <= 32: never for nr <= 66; 32 < n <= 64: never for nr <= 15).  With J=None the plain entry is called.

    state_rows=True (requires J): the constraint-to-go recursion, for any rows -- r_k > nu, rows on the state alone, dependent rows.  Stage k stacks
    Cf = [J_k; Hn_{k+1} [A_k B_k]], splits it by elimination with full pivoting on its u columns (a pivot counts while it exceeds
    rank_tol * max(1, max|Cf|)) into rows of full row rank in u, solved as above, and rows on the state alone, whose independent part is the constraint-to-go
    Hn_k (c_k orthonormal rows, Hn_k x_k = 0); K_k and Pi_k are returned projected with Pz_k = I - Hn_k' Hn_k (u = -K_k x holds for feasible x_k; off the
    subspace it says nothing), Phi = (A-BK)_{p-1} ... (A-BK)_0 Pz_0.  Sweeps stop when the change is <= tol and no c_k changed.  The dict then carries
    Hn [nb,p,nx,nx] (rows beyond c_k zero), cnt [nb,p] int32 (c_k), feas [nb] = info[:, 7] = max_k max(|(Jx - Ju K_k) Pz_k|, |Hn_{k+1} (A_k - B_k K_k) Pz_k|),
    info [nb,12] (8: sum of c_k, 9: max c_k, 10 / 11: smallest accepted / largest rejected pivot of the rank decisions relative to the stage scale) and no
    Lam (the multipliers are not unique); info[:, 5:7] read 0 ("not shown") more often than without state_rows, because the rows enter the elimination scaled
    to S and compete with its diagonal for the pivot.  status 5 (NoFeasibleSubspace): some c_k reached nx; status 4 does not occur.  With every r_k <= nu and full rank the
    result is that of the call without state_rows up to rounding (the pivot order differs).  NotImplementedError for (nx, nu, nr) beyond the 160 KB of
    LDS of its wider layout (the bench stage shape with room for 10 rows takes 61 KB)."""
    use_torch, nb, p, nx, mb = _validate(A, B, H, (('Pi0', Pi0, 'A'),))
    if not (float(tol) >= 0.0) or int(max_sweeps) < 1:
        raise ValueError('periodic_lqr_batch: tol >= 0 and max_sweeps >= 1 expected, got {}, {}'.format(tol, max_sweeps))
    if J is None and (ncnt is not None or ng is not None):
        raise ValueError('periodic_lqr_batch: ncnt / ng describe the rows of J, which is None')
    if state_rows:
        if J is None:
            raise ValueError('periodic_lqr_batch: state_rows=True is the recursion for the rows of J, which is None')
        if isinstance(rank_tol, bool) or not isinstance(rank_tol, (int, float, np.floating)) or not (0.0 < float(rank_tol) < 1.0):
            raise ValueError('periodic_lqr_batch: 0 < rank_tol < 1 expected, got {!r}'.format(rank_tol))
    if J is not None:
        nr, ng = _validate_rows(J, ncnt, ng, use_torch, A, nb, p, nx + mb)
        A, B, H, Pi0, J, ncnt = (_contig(x, use_torch) if x is not ncnt else (x if x is None else (x.contiguous() if use_torch else np.ascontiguousarray(x)))
                                 for x in (A, B, H, Pi0, J, ncnt))
        if state_rows:
            if use_torch:
                import torch
                K, Pi, Phi, Hn, cnt, info = _lib.periodic_lqr_ctg_batch_device(A, B, H, J, ncnt, ng, Pi0, tol, rank_tol, max_sweeps)
                rho = _rho(Phi.cpu().numpy())
                status = info[:, 0].to(torch.int32); sweeps = info[:, 1].to(torch.int32); feas = info[:, 7].clone()
            else:
                K, Pi, Phi, Hn, cnt, info = _lib.periodic_lqr_ctg_batch_host(A, B, H, J, ncnt, ng, Pi0, tol, rank_tol, max_sweeps)
                rho = _rho(Phi)
                status = info[:, 0].astype(np.int32); sweeps = info[:, 1].astype(np.int32); feas = info[:, 7].copy()
            return dict(K=K, Pi=Pi, Phi=Phi, rho=rho, status=status, sweeps=sweeps, info=info, Hn=Hn, cnt=cnt, feas=feas)
        if use_torch:
            import torch
            K, Pi, Phi, Lam, info = _lib.periodic_lqr_rows_batch_device(A, B, H, J, ncnt, ng, Pi0, tol, max_sweeps)
            rho = _rho(Phi.cpu().numpy())
            status = info[:, 0].to(torch.int32); sweeps = info[:, 1].to(torch.int32); feas = info[:, 7].clone()
        else:
            K, Pi, Phi, Lam, info = _lib.periodic_lqr_rows_batch_host(A, B, H, J, ncnt, ng, Pi0, tol, max_sweeps)
            rho = _rho(Phi)
            status = info[:, 0].astype(np.int32); sweeps = info[:, 1].astype(np.int32); feas = info[:, 7].copy()
        return dict(K=K, Pi=Pi, Phi=Phi, rho=rho, status=status, sweeps=sweeps, info=info, Lam=Lam, feas=feas)
    A, B, H, Pi0 = (_contig(x, use_torch) for x in (A, B, H, Pi0))
    if use_torch:
        K, Pi, Phi, info = _lib.periodic_lqr_batch_device(A, B, H, Pi0, tol, max_sweeps)       # (either entry refuses n > 64 before it touches the device)
        rho = _rho(Phi.cpu().numpy())
        import torch
        status = info[:, 0].to(torch.int32); sweeps = info[:, 1].to(torch.int32)
    else:
        K, Pi, Phi, info = _lib.periodic_lqr_batch_host(A, B, H, Pi0, tol, max_sweeps)
        rho = _rho(Phi)
        status = info[:, 0].astype(np.int32); sweeps = info[:, 1].astype(np.int32)
    return dict(K=K, Pi=Pi, Phi=Phi, rho=rho, status=status, sweeps=sweeps, info=info)


def _stack_stages(A, B, Q, R, N, G=None, C=None):
    """The reference's calling style (single matrices or lists of length p, np.matrix / CasADi DM accepted) -> A, B, H [1,p,...] and the rows of
    G, C (as `convexify` takes them: per-stage None allowed in C) as keyword arguments J=, ncnt=, ng= of the batched calls ({} without rows)."""
    arg = {'A': A, 'B': B, 'Q': Q, 'R': R, 'N': N}
    if G is not None:
        arg['G'] = G
    if C is not None:
        arg['C'] = C
    arg = preprocessing.input_checks(arg)
    As = np.stack([_to_array(a) for a in arg['A']]); Bs = np.stack([_to_array(b) for b in arg['B']])
    period, nx, _ = As.shape
    nu = Bs.shape[2]
    Hs = np.zeros((period, nx + nu, nx + nu))
    for k in range(period):
        Qk, Rk, Nk = _to_array(arg['Q'][k]), _to_array(arg['R'][k]), _to_array(arg['N'][k])
        if Qk.shape != (nx, nx) or Rk.shape != (nu, nu) or Nk.shape != (nx, nu) or Bs[k].shape != (nx, nu):
            raise ValueError('periodic_lqr: A (nx,nx), B (nx,nu), Q (nx,nx), R (nu,nu), N (nx,nu) expected at stage {}'.format(k))
        Hs[k, :nx, :nx] = Qk; Hs[k, nx:, nx:] = Rk; Hs[k, :nx, nx:] = Nk; Hs[k, nx:, :nx] = Nk.T
    Gs, Cp, cnt = pack_rows(arg, period, nx + nu)        # (the packing of `convexify`)
    for nm, x in (('G', Gs), ('C', Cp)):
        if x is not None and x.shape[2] != nx + nu:
            raise ValueError('periodic_lqr: rows of {} must have nx + nu = {} columns, got {}'.format(nm, nx + nu, x.shape[2]))
    rows = {}
    if Cp is not None:
        rows = dict(J=(Cp if Gs is None else np.concatenate([Gs, Cp], axis=1))[None], ncnt=np.asarray(cnt, np.int32)[None], ng=0 if Gs is None else Gs.shape[1])
    elif Gs is not None:
        rows = dict(J=Gs[None], ng=Gs.shape[1])
    return As[None], Bs[None], Hs[None], rows


def periodic_lqr(A, B, Q, R, N, tol=1e-13, max_sweeps=5000, G=None, C=None, state_rows=False, rank_tol=1e-9):
    """The gains of one problem in the reference's calling style: A, B, Q, R, N single matrices (p = 1) or lists of length p, as `convexify`
    takes them -> (K_list, Pi_list, rho): p gains K_k (nu x nx, u = -K_k x), p cost-to-go matrices, the closed-loop spectral radius.
    G, C (as `convexify` takes them): the rows held as equalities, see periodic_lqr_batch.  state_rows=True, rank_tol: the constraint-to-go recursion
    (any rows; the gains and cost-to-go matrices are the projected ones, valid on the feasible subspace of each stage).
    RuntimeError when the recursion did not converge (status of periodic_lqr_batch != 0)."""
    As, Bs, Hs, rows = _stack_stages(A, B, Q, R, N, G, C)
    if state_rows:
        if not rows:
            raise ValueError('periodic_lqr: state_rows=True is the recursion for the rows G / C, which are None')
        rows.update(state_rows=True, rank_tol=rank_tol)
    r = periodic_lqr_batch(As, Bs, Hs, tol=tol, max_sweeps=max_sweeps, **rows)
    st = int(r['status'][0])
    if st != 0:
        raise RuntimeError('periodic_lqr: Riccati recursion ended with status {} ({}) after {} sweeps'.format(st, STATUS_NAMES.get(st), int(r['sweeps'][0])))
    p = As.shape[1]
    return [r['K'][0, k].copy() for k in range(p)], [r['Pi'][0, k].copy() for k in range(p)], float(r['rho'][0])


def feedback_equivalence_batch(A, B, H, Hc, P=None, tol=1e-13, max_sweeps=5000, J=None, ncnt=None, ng=None, state_rows=False, rank_tol=1e-9):
    """The certificate: gains of the LQ problems on H and on Hc (two recursions), compared.  A, B, H as in periodic_lqr_batch, Hc [nb,p,n,n]
    (the `Hc` of convexify_batch, or H + dHc), numpy or torch GPU tensors.  Returns dict: dK [nb] = max_k max|K_k(H) - K_k(Hc)|,
    dK_rel = dK / max(1, max|K(Hc)|), rho_H, rho_Hc (numpy), status_H, status_Hc, sweeps_H, sweeps_Hc, posdef_H (info[6] of the H side: 1.0 if S was positive definite on its whole path), K, Kc.

    P [nb,p,nx,nx] (optional): the `P` of the convexification.  With the supplement map of the library (tmpc_supplement_batch_host, reference convexifier.py:191-194),
    Hc_k = H_k + [A_k B_k]' P_{k+1} [A_k B_k] - diag(P_k, 0), so the H-recursion started at Pi0 = +P is the Hc-recursion started at zero
    shifted by P, iterate by iterate (Pi_k(H) = Pi_k(Hc) + P_k): the H side then solves the positive definite S of the Hc side instead of
    the indefinite one it meets on the way from zero.  (The sweep counts agree unless convergence is slow: the stop measure divides by
    max(1, max|Pi_k|), which the shift changes -- c1 stops at sweep 211 from P and at 214 on the Hc side.)

    What it says: for the plain model (Step 1 without rows) dK at rounding level and both rho < 1 certify that dHc has the calH(P) structure
    and that both schemes stabilise.  It does NOT say that kappa is minimal (the SDP may be solved badly and still pass).  After Step 3
    (`force`) dHc contains the regularisation T_k, the gains differ on purpose and dK MEASURES what T_k changed.  The models with rows (Step 1 with
    G, Step 2) are covered when the rows of the solve are passed as J / ncnt / ng (see periodic_lqr_batch): both recursions then hold
    J_k [x_k; u_k] = 0, the term J_k' diag(phi_k) J_k of Hc drops out and dK is at rounding level again (without J the unconstrained gains of H and
    Hc differ by design once a multiplier is non-zero -- a wrong alarm); the dict gains feas_H, feas_Hc (max|Jx - Ju K_k|), convex_Hc (info[6] of the
    Hc side: every stage problem shown convex) and Lam, Lamc.  After Step 3 with rows dK measures T_k as it does without rows.  Not covered: rows
    that constrain the state alone (Ju without full row rank: status 2) and stages with more rows than inputs (status 4) -- unless state_rows=True.

    state_rows=True, rank_tol (requires J): both recursions are the constraint-to-go recursion of periodic_lqr_batch, which serves those cases too.  dK is
    then taken on the projected gains K_k Pz_k (the gains on the feasible subspaces), the dict carries subspace_diff [nb] = max_k max|Pz_k(H side) -
    Pz_k(Hc side)| (the subspaces depend on A, B and the rows only: it must be at rounding level, and dK means nothing where it is not), cnt, cntc, Hn, Hnc
    instead of Lam, Lamc; convex_Hc is reported but seldom 1 (see periodic_lqr_batch).  Not covered: an empty feasible subspace (status 5) and shapes beyond the LDS layout."""
    use_torch, nb, p, nx, mb = _validate(A, B, H, (('Hc', Hc, 'H'), ('P', P, 'A')))
    rows = {} if J is None and ncnt is None and ng is None else dict(J=J, ncnt=ncnt, ng=ng)
    if state_rows:
        rows.update(state_rows=True, rank_tol=rank_tol)             # (without J: the ValueError of periodic_lqr_batch)
    rH = periodic_lqr_batch(A, B, H, Pi0=P, tol=tol, max_sweeps=max_sweeps, **rows)
    rC = periodic_lqr_batch(A, B, Hc, tol=tol, max_sweeps=max_sweeps, **rows)
    d = (rH['K'] - rC['K']).abs() if use_torch else np.abs(rH['K'] - rC['K'])
    kc = rC['K'].abs() if use_torch else np.abs(rC['K'])
    if use_torch:
        dK = d.reshape(nb, -1).max(dim=1).values.cpu().numpy(); kmax = kc.reshape(nb, -1).max(dim=1).values.cpu().numpy()
        posdef = rH['info'][:, 6].cpu().numpy()
    else:
        dK = d.reshape(nb, -1).max(axis=1); kmax = kc.reshape(nb, -1).max(axis=1)
        posdef = rH['info'][:, 6].copy()
    out = dict(dK=dK, dK_rel=dK / np.maximum(1.0, kmax), rho_H=rH['rho'], rho_Hc=rC['rho'], status_H=rH['status'], status_Hc=rC['status'],
               sweeps_H=rH['sweeps'], sweeps_Hc=rC['sweeps'], posdef_H=posdef, K=rH['K'], Kc=rC['K'])
    if rows:
        host = (lambda x: x.cpu().numpy()) if use_torch else (lambda x: x.copy())
        out.update(feas_H=host(rH['feas']), feas_Hc=host(rC['feas']), convex_Hc=host(rC['info'][:, 6]))
        if state_rows:
            out.update(subspace_diff=_subspace_diff(rH['Hn'], rC['Hn'], use_torch), cnt=rH['cnt'], cntc=rC['cnt'], Hn=rH['Hn'], Hnc=rC['Hn'])
        else:
            out.update(Lam=rH['Lam'], Lamc=rC['Lam'])
    return out


def feedback_equivalence(A, B, Q, R, N, dHc, tol=1e-13, max_sweeps=5000, G=None, C=None, state_rows=False, rank_tol=1e-9):
    """feedback_equivalence_batch for one problem in the calling style of `convexify`: dHc is its first return value (list of p supplements,
    Hc_k = H_k + dHc_k).  Returns the dict of the batched call with scalars for dK, dK_rel, rho_H, rho_Hc, status_H, status_Hc and lists of
    p gains for K, Kc.  G, C: the rows `convexify` was called with (then also feas_H, feas_Hc, convex_Hc as scalars).  state_rows=True, rank_tol: the
    constraint-to-go recursion on both sides (any rows; also subspace_diff as a scalar and cnt, cntc as lists of p counts)."""
    As, Bs, Hs, rows = _stack_stages(A, B, Q, R, N, G, C)
    dH = np.stack([_to_array(d) for d in (dHc if isinstance(dHc, (list, tuple)) else [dHc])])[None]      # (convexify returns a list also at p = 1)
    if dH.shape != Hs.shape:
        raise ValueError('feedback_equivalence: dHc must hold p matrices (nx+nu, nx+nu), got {}'.format(dH.shape[1:]))
    if state_rows:
        if not rows:
            raise ValueError('feedback_equivalence: state_rows=True is the recursion for the rows G / C, which are None')
        rows.update(state_rows=True, rank_tol=rank_tol)
    r = feedback_equivalence_batch(As, Bs, Hs, Hs + dH, tol=tol, max_sweeps=max_sweeps, **rows)
    p = As.shape[1]
    out = {k: (float(v[0]) if k.startswith(('dK', 'rho', 'posdef', 'feas', 'convex', 'subspace')) else int(v[0])) for k, v in r.items()
           if k not in ('K', 'Kc', 'Lam', 'Lamc', 'Hn', 'Hnc', 'cnt', 'cntc')}
    if state_rows:
        out['cnt'] = [int(c) for c in r['cnt'][0]]; out['cntc'] = [int(c) for c in r['cntc'][0]]
    out['K'] = [r['K'][0, k].copy() for k in range(p)]; out['Kc'] = [r['Kc'][0, k].copy() for k in range(p)]
    return out


# ----------------------------------------------------------------------------- finite horizon
TERMINAL = {'cost': 0, 'constraint': 1}


def _relabel(fn, who, *a):
    try:
        return fn(*a)
    except ValueError as e:
        raise ValueError(str(e).replace('periodic_lqr_batch', who)) from None


def _validate_horizon(who, horizon, terminal, phases, p, rank_tol):
    """horizon, terminal, phases, rank_tol before any device call -> (N, terminal code, phases as a numpy int32 array or None)."""
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or int(horizon) < 1:
        raise ValueError('{}: horizon must be an int >= 1, got {!r}'.format(who, horizon))
    if not isinstance(terminal, str) or terminal not in TERMINAL:
        raise ValueError("{}: terminal must be 'constraint' (x_N = 0) or 'cost', got {!r}".format(who, terminal))
    if isinstance(rank_tol, bool) or not isinstance(rank_tol, (int, float, np.floating)) or not (0.0 < float(rank_tol) < 1.0):
        raise ValueError('{}: 0 < rank_tol < 1 expected, got {!r}'.format(who, rank_tol))
    if phases is not None:
        if _is_torch(phases):
            phases = phases.cpu().numpy()
        ph = np.asarray(phases)
        if ph.ndim != 1 or ph.size < 1 or ph.dtype.kind not in 'iu':
            raise ValueError('{}: phases must be a non-empty list of ints (None: all p phases), got {!r}'.format(who, phases))
        if (ph < 0).any() or (ph >= p).any():
            raise ValueError('{}: phases must lie in 0 .. p - 1 = {}, got {}'.format(who, p - 1, ph.tolist()))
        phases = np.ascontiguousarray(ph, dtype=np.int32)
    return int(horizon), TERMINAL[terminal], phases


def horizon_lqr_batch(A, B, H, horizon, terminal='constraint', Pf=None, phases=None, J=None, ncnt=None, ng=None, rank_tol=1e-9, return_all=False):
    """First-order feedback of the horizon-N LQ problems on nb p-periodic models, from every starting phase: for problem b and phase k0 one backward pass
    j = horizon-1 ... 0 over the stages k = (k0 + j) mod p (horizon may be smaller than, equal to or larger than p), started from the terminal weight
    Pi_N = Pf[b, (k0 + N) mod p] (Pf [nb,p,nx,nx]; None: zero) and

        terminal='cost':        nothing else;
        terminal='constraint':  x_N = 0, i.e. the constraint-to-go Hn_N = I (a general terminal operator, the reference's p_operator, is not provided).

    A, B, H, J, ncnt, ng, rank_tol as in periodic_lqr_batch(..., state_rows=True): every stage is the constraint-to-go stage, so any rows are served and J=None
    is allowed (under a terminal constraint the constraint-to-go is there without rows).  phases: list of starting phases (None: all p, in order).
    numpy arrays run through the host entry; torch tensors on a GPU through the device entry (torch tensors out, the inputs are not copied).

    Returns dict: K0 [nb,nph,nu,nx] (u_0 = -K0 x_0 for feasible x_0: projected with Pz_0 = I - Hn0' Hn0), Pi0 [nb,nph,nx,nx] (cost-to-go of x_0, projected),
    Hn0 [nb,nph,nx,nx] (c_0 orthonormal rows, Hn0 x_0 = 0: the x_0 from which the horizon problem is feasible; rows beyond c_0 zero), cnt0 [nb,nph] int32,
    status [nb,nph] (0 done, 2 singular stage system, 3 non-finite, 5 no feasible subspace: a computed c_j reached nx; 1 and 4 do not occur), feas [nb,nph] =
    info[..., 7] = max_j max(|(Jx - Ju K_j) Pz_j|, |Hn_{j+1} (A - B K_j) Pz_j|), info [nb,nph,12] (1: N, 2: stages finished, else the slots of the ctg entry),
    phases (numpy int32).  Where status >= 2: K0, Pi0 NaN, Hn0 zero, cnt0 the count at the failing stage.  One (problem, phase) never affects another.
    return_all=True adds Kall [nb,nph,N,nu,nx] and cntall [nb,nph,N], the gains and counts of every stage of every pass (large: nb nph N nu nx doubles;
    NaN / -1 at the stages a failed pass did not finish).  ValueError: shapes, dtypes, horizon < 1, a phase outside 0 .. p-1, terminal;
    NotImplementedError: (nx, nu, nr) beyond the 160 KB LDS layout of the ctg entry, more than 65535 phases."""
    who = 'horizon_lqr_batch'
    use_torch, nb, p, nx, mb = _relabel(_validate, who, A, B, H, (('Pf', Pf, 'A'),))
    N, term, phases = _validate_horizon(who, horizon, terminal, phases, p, rank_tol)
    if J is None and (ncnt is not None or ng is not None):
        raise ValueError('{}: ncnt / ng describe the rows of J, which is None'.format(who))
    ng_ = 0
    if J is not None:
        _, ng_ = _relabel(_validate_rows, who, J, ncnt, ng, use_torch, A, nb, p, nx + mb)
    A, B, H, Pf, J = (_contig(x, use_torch) for x in (A, B, H, Pf, J))
    if ncnt is not None:
        ncnt = ncnt.contiguous() if use_torch else np.ascontiguousarray(ncnt)
    entry = _lib.horizon_lqr_batch_device if use_torch else _lib.horizon_lqr_batch_host
    K0, Pi0, Hn0, cnt0, Kall, cntall, info = entry(A, B, H, J, ncnt, ng_, N, phases, term, Pf, rank_tol, bool(return_all))
    if use_torch:
        import torch
        status = info[..., 0].to(torch.int32); feas = info[..., 7].clone()
    else:
        status = info[..., 0].astype(np.int32); feas = info[..., 7].copy()
    out = dict(K0=K0, Pi0=Pi0, Hn0=Hn0, cnt0=cnt0, status=status, feas=feas, info=info, phases=np.arange(p, dtype=np.int32) if phases is None else phases)
    if return_all:
        out.update(Kall=Kall, cntall=cntall)
    return out


def horizon_equivalence_batch(A, B, H, Hc, horizon, P=None, terminal='constraint', Pf=None, phases=None, J=None, ncnt=None, ng=None, rank_tol=1e-9):
    """The finite-horizon certificate: K_0 of the horizon-N problems on H and on Hc (two passes per phase), compared.  Arguments as in horizon_lqr_batch, Hc
    [nb,p,n,n] and P [nb,p,nx,nx], the `P` of the convexification: Hc_k = H_k + [A_k B_k]' P_{k+1} [A_k B_k] - diag(P_k, 0) (+ J_k' diag(phi_k) J_k, which
    vanishes on the rows).  The cost of the H problem is that of the Hc problem plus x_0' P_k0 x_0 - x_N' P_{k0+N} x_N, so the two are the same problem when
    the H side carries the terminal weight Pf + P[(k0 + N) mod p] and the Hc side Pf: that is what is run.  terminal='cost' therefore needs P (ValueError
    without it: dK0 would measure the mismatch of the terminal weights, O(1) at N = 1 and fading with N).  With terminal='constraint' x_N = 0 makes the
    terminal weight irrelevant in exact arithmetic and P is optional; when given it is used, because it keeps S of the H side convex on the way.

    Returns dict of numpy arrays [nb,nph]: dK0 = max|K0(H) - K0(Hc)| on the projected gains, dK0_rel = dK0 / max(1, max|K0(Hc)|), subspace_diff =
    max|Pz_0(H side) - Pz_0(Hc side)| (the subspaces depend on A, B and the rows only: rounding level, and dK0 means nothing where it is not), cnt0_H,
    cnt0_Hc, status_H, status_Hc, feas_H, feas_Hc; and K0, K0c as the entries returned them.  dK0 is NaN where a side ended with status >= 2.  Not covered: an
    empty feasible subspace (status 5), a general terminal operator, shapes beyond the LDS layout."""
    who = 'horizon_equivalence_batch'
    use_torch, nb, p, nx, mb = _relabel(_validate, who, A, B, H, (('Hc', Hc, 'H'), ('P', P, 'A'), ('Pf', Pf, 'A')))
    _validate_horizon(who, horizon, terminal, phases, p, rank_tol)
    if terminal == 'cost' and P is None:
        raise ValueError("{}: terminal='cost' needs P: the H side must carry the terminal weight Pf + P[(k0 + N) mod p] for the two problems to be "
                         'the same'.format(who))
    PfH = Pf if P is None else (P if Pf is None else Pf + P)
    kw = dict(terminal=terminal, phases=phases, J=J, ncnt=ncnt, ng=ng, rank_tol=rank_tol)
    rH = horizon_lqr_batch(A, B, H, horizon, Pf=PfH, **kw)
    rC = horizon_lqr_batch(A, B, Hc, horizon, Pf=Pf, **kw)
    nph = rH['K0'].shape[1]
    host = (lambda x: x.cpu().numpy()) if use_torch else (lambda x: np.array(x))
    if use_torch:
        import torch
        d = (rH['K0'] - rC['K0']).abs().reshape(nb, nph, -1).max(dim=2).values; kmax = rC['K0'].abs().reshape(nb, nph, -1).max(dim=2).values
        sd = (torch.einsum('bkji,bkjl->bkil', rH['Hn0'], rH['Hn0']) - torch.einsum('bkji,bkjl->bkil', rC['Hn0'], rC['Hn0'])).abs().reshape(nb, nph, -1).max(dim=2).values
    else:
        d = np.abs(rH['K0'] - rC['K0']).reshape(nb, nph, -1).max(axis=2); kmax = np.abs(rC['K0']).reshape(nb, nph, -1).max(axis=2)
        sd = np.abs(np.einsum('bkji,bkjl->bkil', rH['Hn0'], rH['Hn0']) - np.einsum('bkji,bkjl->bkil', rC['Hn0'], rC['Hn0'])).reshape(nb, nph, -1).max(axis=2)
    dK0, kmax = host(d), host(kmax)
    with np.errstate(invalid='ignore'):
        rel = dK0 / np.maximum(1.0, kmax)
    return dict(dK0=dK0, dK0_rel=rel, subspace_diff=host(sd), cnt0_H=host(rH['cnt0']), cnt0_Hc=host(rC['cnt0']), status_H=host(rH['status']),
                status_Hc=host(rC['status']), feas_H=host(rH['feas']), feas_Hc=host(rC['feas']), K0=rH['K0'], K0c=rC['K0'], phases=rH['phases'])


def _stack_weights(X, p, nx, name):
    """A single (nx, nx) matrix or a list of p of them (None passes through) -> [1,p,nx,nx]."""
    if X is None:
        return None
    Xs = [_to_array(x) for x in X] if isinstance(X, (list, tuple)) else [_to_array(X)] * p
    if len(Xs) != p or any(x.shape != (nx, nx) for x in Xs):
        raise ValueError('horizon_lqr: {} must be one (nx, nx) matrix or a list of p = {} of them'.format(name, p))
    return np.ascontiguousarray(np.stack(Xs)[None], dtype=np.float64)


def horizon_lqr(A, B, Q, R, N, horizon, terminal='constraint', Pf=None, phases=None, G=None, C=None, rank_tol=1e-9):
    """K_0 of one model in the reference's calling style (N is the cross term, as in periodic_lqr; the horizon is `horizon`): A, B, Q, R, N single matrices
    (p = 1) or lists of length p, G, C the rows as `convexify` takes them, Pf one (nx, nx) matrix or a list of p -> (K0_list, Pi0_list, cnt0_list), one entry
    per starting phase (phases=None: all p): the projected gain (nu x nx, u_0 = -K_0 x_0 on the feasible x_0), the projected cost-to-go, the count c_0.
    RuntimeError when a pass did not finish (status of horizon_lqr_batch != 0)."""
    As, Bs, Hs, rows = _stack_stages(A, B, Q, R, N, G, C)
    r = horizon_lqr_batch(As, Bs, Hs, horizon, terminal=terminal, Pf=_stack_weights(Pf, As.shape[1], As.shape[2], 'Pf'), phases=phases, rank_tol=rank_tol, **rows)
    bad = np.nonzero(r['status'][0])[0]
    if bad.size:
        st = int(r['status'][0, bad[0]])
        raise RuntimeError('horizon_lqr: the pass from phase {} ended with status {} ({}) after {} of {} stages'.format(
            int(r['phases'][bad[0]]), st, STATUS_NAMES.get(st), int(r['info'][0, bad[0], 2]), int(horizon)))
    nph = r['K0'].shape[1]
    return [r['K0'][0, i].copy() for i in range(nph)], [r['Pi0'][0, i].copy() for i in range(nph)], [int(c) for c in r['cnt0'][0]]


def horizon_equivalence(A, B, Q, R, N, dHc, horizon, P=None, terminal='constraint', Pf=None, phases=None, G=None, C=None, rank_tol=1e-9):
    """horizon_equivalence_batch for one model in the calling style of `convexify`: dHc is its first return value (list of p supplements, Hc_k = H_k + dHc_k),
    P its second (list of p matrices, or None), G, C the rows it was called with.  Returns the dict of the batched call with lists over the starting phases
    (floats for dK0, dK0_rel, subspace_diff, feas_H, feas_Hc; ints for cnt0_H, cnt0_Hc, status_H, status_Hc; matrices for K0, K0c)."""
    As, Bs, Hs, rows = _stack_stages(A, B, Q, R, N, G, C)
    dH = np.stack([_to_array(d) for d in (dHc if isinstance(dHc, (list, tuple)) else [dHc])])[None]
    if dH.shape != Hs.shape:
        raise ValueError('horizon_equivalence: dHc must hold p matrices (nx+nu, nx+nu), got {}'.format(dH.shape[1:]))
    p, nx = As.shape[1], As.shape[2]
    r = horizon_equivalence_batch(As, Bs, Hs, Hs + dH, horizon, P=_stack_weights(P, p, nx, 'P'), terminal=terminal, Pf=_stack_weights(Pf, p, nx, 'Pf'),
                                  phases=phases, rank_tol=rank_tol, **rows)
    out = {}
    for k, v in r.items():
        if k in ('K0', 'K0c'):
            out[k] = [v[0, i].copy() for i in range(v.shape[1])]
        elif k == 'phases':
            out[k] = [int(x) for x in v]
        else:
            out[k] = [(int(x) if k.startswith(('cnt', 'status')) else float(x)) for x in v[0]]
    return out
