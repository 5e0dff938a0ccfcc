"""Plain numpy reference of the block factorisation of tunempc_amd/csrc/tmpc_cr.h, walking the library's own elimination schedule
(`tunempc_amd._lib.cr_schedule`, host only) -- TEST INFRASTRUCTURE ONLY.  numpy plays the kernels: Cholesky of the eliminated nodes,
O_x = T[x,i] L_i^-T, D_s -= O_s O_s', fill T[x,y] (-)= O_x O_y', and the forward / backward substitutions in the same order, under one
of three precision policies that mirror what the kernels do for a problem:

  fp64         everything in fp64 (k_cr_potrf_dma, k_cr_trsm_dma, k_cr_update_dma);
  f32_updates  Cholesky and O = E L^-T in fp64, O rounded to float32 (the O32 copy written by k_cr_trsm_dma), the updates and fills as
               float32 products with float32 accumulation (k_cr_update_dma_f32) subtracted from / stored into the fp64 blocks, the
               substitutions as fp64 products on the float32 O;
  f32_trsm     additionally O computed in float32 from E and L rounded to float32 (k_cr_trsm_dma_f32).

Also here: a generator of SPD block-cyclic-tridiagonal systems with a prescribed condition number, the dense matrix in the arithmetic of
the truth (longdouble), normwise backward errors in longdouble, and an exact-to-rounding residual of a double-double solution."""
import math

import numpy as np
import scipy.linalg as sla

POLICIES = ('fp64', 'f32_updates', 'f32_trsm')


def spd_cyclic(rng, p, d):
    """cond(T) ~ 10: T = I + sum_k J_k' J_k with J_k = [E_k F_k] on blocks (k, k+1).  Returns D, Ccpl (Ccpl[k] = T[block k, block k+1]), dense T."""
    E = rng.standard_normal((p, 2 * d, d)) / np.sqrt(2 * d); F = rng.standard_normal((p, 2 * d, d)) / np.sqrt(2 * d)
    D = np.stack([np.eye(d) for _ in range(p)]); Cc = np.zeros((p, d, d))
    for k in range(p):
        D[k] += E[k].T @ E[k]; D[(k + 1) % p] += F[k].T @ F[k]; Cc[k] = E[k].T @ F[k]
    return D, Cc, dense(D, Cc)


def dense(D, Cc, dtype=np.float64):
    """the dense matrix in arithmetic `dtype` (p = 1 and p = 2 add blocks to each other: not exact in fp64, so the truth assembles in longdouble)"""
    p, d, _ = D.shape
    T = np.zeros((p * d, p * d), dtype)
    for k in range(p):
        kn = (k + 1) % p
        T[k*d:(k+1)*d, k*d:(k+1)*d] += D[k].astype(dtype)
        T[k*d:(k+1)*d, kn*d:(kn+1)*d] += Cc[k].astype(dtype); T[kn*d:(kn+1)*d, k*d:(k+1)*d] += Cc[k].T.astype(dtype)
    return T


def _gram_system(Q, p, d, c):
    D = np.zeros((p, d, d)); Cc = np.zeros((p, d, d))
    w = np.logspace(0.0, -c, 2 * d)
    for k in range(p):
        G = (Q[k] * w) @ Q[k].T
        G = 0.5 * (G + G.T)
        D[k] += G[:d, :d]; D[(k + 1) % p] += G[d:, d:]; Cc[k] = G[:d, d:]
    return D, Cc


def spd_cyclic_cond(rng, p, d, cond):
    """A system with cond_2(T) within a factor 2 of `cond`: per edge a Gram term Q diag(logspace(0, -c)) Q' on the two blocks it couples (Q random
    orthogonal, 2d x 2d).  The sum of overlapping terms is better conditioned than one term, so c is corrected twice from the measured cond(T).
    Returns D, Ccpl, the measured cond_2(T), ||T||_2."""
    Q = np.stack([np.linalg.qr(rng.standard_normal((2 * d, 2 * d)))[0] for _ in range(p)])
    c = math.log10(cond)
    for _ in range(4):
        D, Cc = _gram_system(Q, p, d, c)
        ev = np.linalg.eigvalsh(dense(D, Cc))
        got = ev[-1] / ev[0] if ev[0] > 0 else np.inf
        if 0.5 * cond <= got <= 2.0 * cond:
            break
        c += math.log10(cond) - (math.log10(got) if np.isfinite(got) else c + 2)
    return D, Cc, float(got), float(ev[-1])


def reference(sched, D, Cc, rhs, policy='fp64'):
    """Factor + solve along the schedule.  rhs [p, d] or [p, d, nc].  Returns dict: L {node: L_i}, slots {slot: block} (edge and fill slots as the
    substitutions use them: O factors once solved -- the float32 values, widened, under the float32 policies), pre {slot: E}, the block each solve
    started from, solved (set of slots that hold an O factor), x, top (highest slot number)."""
    assert policy in POLICIES
    f32u = policy != 'fp64'; f32t = policy == 'f32_trsm'
    p, d, _ = D.shape
    D = D.copy()
    slots = {}
    for k in range(p):                       # k_schur: slot k in the orientation of the schedule
        slots[k] = Cc[k].copy() if sched['orient'][k] else Cc[k].T.copy()
    if sched['prep'] == 1:
        D[0] = D[0] + slots[0] + slots[0].T
    elif sched['prep'] == 2:
        slots[0] = slots[0] + slots[1]
    L = {}; pre = {}
    written = set()
    f32 = np.float32
    for (eoff, nelim, uoff, nupd) in sched['levels']:
        recs = sched['elim'][eoff:eoff + nelim]
        for r in recs:                       # k_cr_potrf (raises LinAlgError on a non-positive pivot)
            L[r[0]] = np.linalg.cholesky(D[r[0]])
        for r in recs:                       # k_cr_trsm
            for e in (r[3], r[4]):
                if e >= 0:
                    assert e not in written, 'an edge slot is solved twice'
                    written.add(e)
                    pre[e] = slots[e].copy()
                    if f32t:
                        slots[e] = sla.solve_triangular(L[r[0]].astype(f32), slots[e].astype(f32).T, lower=True, check_finite=False).T.astype(np.float64)
                    else:
                        slots[e] = sla.solve_triangular(L[r[0]], slots[e].T, lower=True).T
                        if f32u:
                            slots[e] = slots[e].astype(f32).astype(np.float64)
        prod = (lambda a, b: (a.astype(f32) @ b.astype(f32).T).astype(np.float64)) if f32u else (lambda a, b: a @ b.T)
        targets = set()
        for u in sched['upd'][uoff:uoff + nupd]:     # k_cr_update, symmetric part
            assert u[0] not in targets, 'two work items update the same diagonal block'
            targets.add(u[0])
            for e in (u[1], u[3]):
                if e >= 0:
                    D[u[0]] -= prod(slots[e], slots[e])
        fills = set()
        for r in recs:                       # k_cr_update, fill edges
            if r[5] < 0:
                continue
            assert r[5] not in fills, 'two fills meet in one block'
            fills.add(r[5])
            ox, oy = (slots[r[4]], slots[r[3]]) if r[6] else (slots[r[3]], slots[r[4]])
            if r[7]:
                slots[r[5]] = slots[r[5]] - prod(ox, oy)
            else:
                assert r[5] not in slots
                slots[r[5]] = -prod(ox, oy)
    z = np.array(rhs, dtype=np.float64)
    for (eoff, nelim, uoff, nupd) in sched['levels']:
        for r in sched['elim'][eoff:eoff + nelim]:
            z[r[0]] = sla.solve_triangular(L[r[0]], z[r[0]], lower=True)
        for u in sched['upd'][uoff:uoff + nupd]:
            for e, src in ((u[1], u[2]), (u[3], u[4])):
                if e >= 0:
                    z[u[0]] -= slots[e] @ z[src]
    for (eoff, nelim, uoff, nupd) in sched['levels'][::-1]:
        for r in sched['elim'][eoff:eoff + nelim]:
            for e, nb in ((r[3], r[1]), (r[4], r[2])):
                if e >= 0:
                    z[r[0]] -= slots[e].T @ z[nb]
            z[r[0]] = sla.solve_triangular(L[r[0]].T, z[r[0]], lower=False)
    return dict(L=L, slots=slots, pre=pre, solved=written, x=z, top=max(slots) if slots else 0)


def emulate(sched, D, Cc, rhs):
    """the fp64 policy: (x, highest slot number)"""
    r = reference(sched, D, Cc, rhs, 'fp64')
    return r['x'], r['top']


# ---------------------------------------------------------------------------------- error measures
def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def backward_error(Tl, x, b, norm2):
    """normwise backward error ||T x - b||_2 / (||T||_2 ||x||_2 + ||b||_2), residual and norms of the vectors in longdouble; Tl the longdouble dense matrix,
    norm2 = ||T||_2 (the 2-norm, so that cond_2(T) times this number bounds the forward error -- with the Frobenius norm it would not)"""
    x = np.asarray(x, np.longdouble).ravel(); b = np.asarray(b, np.longdouble).ravel()
    r = Tl @ x - b
    return float(np.sqrt(r @ r) / (norm2 * np.sqrt(x @ x) + np.sqrt(b @ b)))


def solve_truth(Tl, b):
    """dense solve in longdouble: fp64 LU solve + iterative refinement with longdouble residuals to convergence (accurate while cond(T) u_64 < 1)"""
    T64 = Tl.astype(np.float64)
    lu = sla.lu_factor(T64)
    b = np.asarray(b, np.longdouble).reshape(Tl.shape[0], -1)
    x = np.zeros_like(b)
    for _ in range(40):
        r = b - Tl @ x
        dx = sla.lu_solve(lu, r.astype(np.float64)).astype(np.longdouble)
        x = x + dx
        if np.abs(dx).max() <= 4 * np.finfo(np.longdouble).eps * np.abs(x).max():
            break
    return x


def block_trsm_residual(O, L, E):
    """||O L' - E||_F / (||O||_F ||L||_F) in longdouble: how well a computed O solves O L' = E"""
    Ol = np.asarray(O, np.longdouble); Ll = np.asarray(L, np.longdouble); El = np.asarray(E, np.longdouble)
    R = Ol @ Ll.T - El
    return float(np.sqrt((R * R).sum()) / (np.sqrt((Ol * Ol).sum()) * np.sqrt((Ll * Ll).sum())))


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    pr = a * b
    ah, al = _split(a); bh, bl = _split(b)
    return pr, ((ah * bh - pr) + ah * bl + al * bh) + al * bl


def dd_residual(D, Cc, xh, xl, b, Dlo=None, Clo=None):
    """r = b - T (xh + xl), every row correctly rounded: each product of fp64 words is split exactly (Dekker) and a row is summed with math.fsum.
    T is never assembled (blocks that coincide at p = 1, 2 are separate terms of the sum); the low words of T enter to first order (lo x lo is below
    2^-104 of a term).  Returns r [p, d]."""
    p, d, _ = D.shape
    z = np.zeros_like(D)
    Dlo = z if Dlo is None else Dlo; Clo = z if Clo is None else Clo
    r = np.zeros((p, d))
    rows = [[] for _ in range(p)]
    for k in range(p):
        kn = (k + 1) % p
        rows[k].append((D[k], Dlo[k], k)); rows[k].append((Cc[k], Clo[k], kn)); rows[kn].append((Cc[k].T, Clo[k].T, k))
    for k in range(p):
        parts = [np.asarray(b[k], np.float64)[:, None]]
        for (Mh, Ml, j) in rows[k]:
            pr, er = _two_prod(Mh, xh[j][None, :])
            p2, e2 = _two_prod(Mh, xl[j][None, :])
            p3, e3 = _two_prod(Ml, xh[j][None, :])
            parts += [-pr, -er, -p2, -e2, -p3, -e3, -(Ml * xl[j][None, :])]
        allp = np.concatenate(parts, axis=1)
        r[k] = [math.fsum(row) for row in allp]
    return r


def reference_dd(sched, D, Cc, rhs, Dlo=None, Clo=None):
    """The same walk in double-double (oracle/ddnum.py: the numpy twin of tmpc_dd.h).  Returns dict(L {node: DD}, slots {slot: DD}, x DD [p, d])."""
    import ddnum as dn
    p, d, _ = D.shape
    Dd = dn.DD(D.copy(), None if Dlo is None else Dlo.copy())
    Cd = dn.DD(Cc.copy(), None if Clo is None else Clo.copy())
    Dn = {k: Dd[k] for k in range(p)}
    slots = {k: (Cd[k].copy() if sched['orient'][k] else Cd[k].T.copy()) for k in range(p)}
    if sched['prep'] == 1:
        Dn[0] = Dn[0] + (slots[0] + slots[0].T)
    elif sched['prep'] == 2:
        slots[0] = slots[0] + slots[1]
    L = {}
    for (eoff, nelim, uoff, nupd) in sched['levels']:
        recs = sched['elim'][eoff:eoff + nelim]
        for r in recs:
            L[r[0]] = dn.cholesky(Dn[r[0]])
        for r in recs:
            for e in (r[3], r[4]):
                if e >= 0:
                    slots[e] = dn.solve_lower(L[r[0]], slots[e].T).T.copy()
        for u in sched['upd'][uoff:uoff + nupd]:
            for e in (u[1], u[3]):
                if e >= 0:
                    Dn[u[0]] = Dn[u[0]] - dn.matmul_nt(slots[e], slots[e])
        for r in recs:
            if r[5] < 0:
                continue
            ox, oy = (slots[r[4]], slots[r[3]]) if r[6] else (slots[r[3]], slots[r[4]])
            slots[r[5]] = (slots[r[5]] - dn.matmul_nt(ox, oy)) if r[7] else -dn.matmul_nt(ox, oy)
    z = {k: dn.DD(np.array(rhs[k], dtype=np.float64).reshape(d, -1)) for k in range(p)}
    for (eoff, nelim, uoff, nupd) in sched['levels']:
        for r in sched['elim'][eoff:eoff + nelim]:
            z[r[0]] = dn.solve_lower(L[r[0]], z[r[0]])
        for u in sched['upd'][uoff:uoff + nupd]:
            for e, src in ((u[1], u[2]), (u[3], u[4])):
                if e >= 0:
                    z[u[0]] = z[u[0]] - dn.matmul_nt(slots[e], z[src].T)
    for (eoff, nelim, uoff, nupd) in sched['levels'][::-1]:
        for r in sched['elim'][eoff:eoff + nelim]:
            for e, nb in ((r[3], r[1]), (r[4], r[2])):
                if e >= 0:
                    z[r[0]] = z[r[0]] - dn.matmul_nt(slots[e].T, z[nb].T)
            z[r[0]] = dn.solve_lower(L[r[0]], z[r[0]], trans=True)
    xh = np.stack([z[k].hi for k in range(p)]); xl = np.stack([z[k].lo for k in range(p)])
    if np.ndim(rhs) == 2:
        xh = xh[..., 0]; xl = xl[..., 0]
    return dict(L=L, slots=slots, xh=xh, xl=xl)


# ---------------------------------------------------------------------------------- the cases of the kernel-level tests
# (tests/test_gpu_factor_kernels.py runs them on the GPU; tests/test_cr_reference.py checks on the CPU that every policy factors every one of them
#  without a non-positive pivot -- the condition that lets the GPU tests demand nshift == 0 -- and prints the reference's own errors)
# (p, d, target cond(T)); the measured cond(T) is what the tests quote and use
F32_CASES = [(2, 65, 1e2), (3, 129, 1e3), (4, 144, 1e5), (5, 80, 1e4), (8, 160, 1e3), (13, 193, 1e2), (3, 210, 1e5), (3, 300, 1e4), (2, 304, 1e3),
             (3, 320, 3e1), (4, 193, 3e1), (5, 304, 1e2)]
FP64_CASES = [(1, 80, 1e2), (1, 300, 1e5), (2, 65, 1e8), (3, 129, 1e2), (4, 144, 1e5), (5, 210, 1e8), (8, 160, 1e5), (13, 80, 1e2), (3, 320, 1e8),
              (3, 300, 1e5), (2, 330, 1e5), (4, 40, 1e5), (5, 10, 1e5), (2, 12, 1e2), (1, 9, 1e8)]
DD_CASES = [(1, 10, 1e4), (5, 10, 1e12), (3, 78, 1e8), (4, 78, 1e12), (3, 136, 1e4), (2, 136, 1e12), (2, 300, 1e8), (3, 300, 1e12)]
LIST_CASES = [(5, 129, 1e3), (3, 300, 1e4)]        # batches of 6 distinct systems
_CACHE = {}


def case(p, d, cond, nb=1):
    """dict(D, Cc [nb, p, d, d], cond [nb] measured, norm2 [nb] = ||T||_2, b1 [nb, p, d], b3 [nb, p, d, 3]) -- deterministic in (p, d, cond, nb)"""
    key = (p, d, cond, nb)
    if key not in _CACHE:
        rng = np.random.default_rng([p, d, int(round(10 * math.log10(cond))), nb])
        sys_ = [spd_cyclic_cond(rng, p, d, cond) for _ in range(nb)]
        _CACHE[key] = dict(D=np.stack([s[0] for s in sys_]), Cc=np.stack([s[1] for s in sys_]), cond=np.array([s[2] for s in sys_]), norm2=np.array([s[3] for s in sys_]),
                           b1=rng.standard_normal((nb, p, d)), b3=rng.standard_normal((nb, p, d, 3)))
    return _CACHE[key]
