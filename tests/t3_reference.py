"""Plain numpy reference of the Step 3 kernels (tunempc_amd/csrc/tmpc_t3.h: theta_k >= 0, the norm cone (t_k; w c o theta_k) in Q^{m+1}), one function per layer, for
tests/test_t3_reference_cpu.py and tests/test_gpu_t3_kernels.py.  No device, no oracle import.

Every function takes the INPUTS OF ITS OWN LAYER (on the GPU: as read back from the workspace) and returns VB objects: the value in np.longdouble (.v), the
absolute-sum bound (.b) and the number of nested roundings (.m), all three carried through the arithmetic by the class itself:
    a + b, a - b   value a.v +- b.v       bound a.b + b.b                   m = max(a.m, b.m) + 1
    a * b          value a.v b.v          bound a.b b.b                     m = a.m + b.m + 1
    a / b          value a.v / b.v        bound a.b b.b / b.v^2             m = a.m + b.m + 1      (the condition b.b / |b.v| of the divisor multiplies the bound)
    sqrt(a)        value sqrt(a.v)        bound sqrt|a.v| a.b / |a.v|       m = a.m + 1            (likewise)
    sum of K       value, bound summed                                      m = max m + K
A kernel that forms the entry by the same operations in any order (with or without fused multiply-adds) errs by at most gamma_m * bound to first order (Higham,
Accuracy and Stability of Numerical Algorithms, Lemma 3.1, (3.13)); the tests allow 4 gamma_m * bound like tests/schur_reference.py.  The cone quantities that pass
through 1 / sqrt(det u), det u = u0^2 - |u1|^2, get the conditioning kappa(u) = (u0^2 + |u1|^2) / det u from the division and square-root rules: the bound of det u
IS u0^2 + |u1|^2.  An exact input (a device array, a constant of the kernel) has bound |v| and m = 0.

Index conventions: n = nx + mb, entries e = (a, b), a <= b, row-major upper triangle (np.triu_indices), c_e = 1 on the diagonal and the double 1.4142135623730951 off
it (the kernels' constant, not sqrt(2) in extended precision), we_e = 1 / 2; cone vectors of length m + 1 with the epigraph variable first."""
import numpy as np

LD = np.longdouble
SQ2 = 1.4142135623730951


class VB:
    __array_priority__ = 100

    def __init__(self, v, b=None, m=0):
        self.v = np.asarray(v, LD)
        self.b = np.abs(self.v) if b is None else np.asarray(b, LD)
        self.m = int(m)

    @staticmethod
    def of(x):
        return x if isinstance(x, VB) else VB(x)

    def __add__(self, o):
        o = VB.of(o)
        return VB(self.v + o.v, self.b + o.b, max(self.m, o.m) + 1)
    __radd__ = __add__

    def __sub__(self, o):
        o = VB.of(o)
        return VB(self.v - o.v, self.b + o.b, max(self.m, o.m) + 1)

    def __rsub__(self, o):
        return VB.of(o) - self

    def __neg__(self):
        return VB(-self.v, self.b, self.m)

    def __mul__(self, o):
        o = VB.of(o)
        return VB(self.v * o.v, self.b * o.b, self.m + o.m + 1)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = VB.of(o)
        return VB(self.v / o.v, self.b * o.b / (o.v * o.v), self.m + o.m + 1)

    def __rtruediv__(self, o):
        return VB.of(o) / self

    def __getitem__(self, i):
        return VB(self.v[i], self.b[i], self.m)

    def __matmul__(self, o):
        o = VB.of(o)
        return VB(self.v @ o.v, self.b @ o.b, self.m + o.m + 1 + self.v.shape[-1])

    @property
    def T(self):
        return VB(np.swapaxes(self.v, -1, -2), np.swapaxes(self.b, -1, -2), self.m)

    def sum(self, axis=None):
        k = self.v.size if axis is None else self.v.shape[axis]
        return VB(self.v.sum(axis=axis), self.b.sum(axis=axis), self.m + max(k, 1))

    def sqrt(self):
        return VB(np.sqrt(self.v), np.sqrt(np.abs(self.v)) * self.b / np.abs(self.v), self.m + 1)

    def min(self):
        i = int(np.argmin(self.v))
        return self[i]


def cat(parts):
    parts = [VB.of(p) for p in parts]
    return VB(np.concatenate([np.atleast_1d(p.v) for p in parts]), np.concatenate([np.atleast_1d(p.b) for p in parts]), max(p.m for p in parts))


def where(c, a, b):
    a, b = VB.of(a), VB.of(b)
    return VB(np.where(c, a.v, b.v), np.where(c, a.b, b.b), max(a.m, b.m))


def tri(n):
    """-> (a, b, c, we) of the m = n (n + 1) / 2 entries"""
    ta, tb = np.triu_indices(n)
    diag = ta == tb
    return ta, tb, np.where(diag, 1.0, SQ2), np.where(diag, 1.0, 2.0)


def J(u):
    u = VB.of(u)
    return cat([u[0], -u[1:]])


def dot1(u, v):
    return (VB.of(u)[1:] * VB.of(v)[1:]).sum()


def det(u):
    """det u = u0^2 - |u1|^2; its bound is u0^2 + |u1|^2 = kappa(u) det u"""
    u = VB.of(u)
    return u[0] * u[0] - dot1(u, u)


def kappa(u):
    u = np.asarray(u, LD)
    return float((u[0] * u[0] + u[1:] @ u[1:]) / (u[0] * u[0] - u[1:] @ u[1:]))


# ---------------------------------------------------------------------------------------------------------------- k_t3_init
def start(p, n, wr):
    """the starting point on the central path of the norm term -> dict(th, z [scalars, the same for every entry], t, x [m + 1])"""
    _, _, c, _ = tri(n)
    x0 = VB(1.0) / VB(float(p * n))
    q = x0 * float(n) / wr
    ph = q if q.v < 1.0 else VB(1.0)
    an = wr * ph * float(n)
    t0 = 0.5 * (x0 + (x0 * x0 + 4.0 * an * an).sqrt())
    dt = t0 * t0 - an * an
    return dict(th=ph, z=x0 / ph, t=t0, x=cat([x0 * t0 / dt, -(x0 * wr * VB(c) * ph) / dt]), x0=x0)


# ---------------------------------------------------------------------------------------------------------------- the slack and the scaling (k_t3_pre)
def slack(t, th, wr, n):
    """s = (t; w c o theta)"""
    _, _, c, _ = tri(n)
    return cat([VB(t), VB(wr * c, m=1) * VB(th)])


def scaling(s, x):
    """Nesterov-Todd scaling of the pair (slack s, multiplier x): -> (beta, v) with W = beta (2 v v' - J), W x = W^-1 s"""
    s, x = VB.of(s), VB.of(x)
    sdet, xdet = det(s), det(x)
    rs, rx = 1.0 / sdet.sqrt(), 1.0 / xdet.sqrt()
    xs = x[0] * s[0] + dot1(x, s)
    gam = (0.5 * (1.0 + xs * rs * rx)).sqrt()
    wb0 = (s[0] * rs + x[0] * rx) / (2.0 * gam)
    nv = 1.0 / (2.0 * (wb0 + 1.0)).sqrt()
    beta = (sdet / xdet).sqrt().sqrt()
    v = cat([nv * (wb0 + 1.0), nv * (s[1:] * rs - x[1:] * rx) / (2.0 * gam)])
    return beta, v


def scaled_point(beta, v, x):
    """lambda = W x"""
    beta, v, x = VB.of(beta), VB.of(v), VB.of(x)
    vx = v[0] * x[0] + dot1(v, x)
    return beta * (2.0 * v * vx - J(x))


def w2inv(beta, v):
    """W^-2 = (I + 4 (v'v) Jv Jv' - 2 (Jv v' + v Jv')) / beta^2, dense [m + 1, m + 1]"""
    beta, v = VB.of(beta), VB.of(v)
    jv = J(v)
    vsq = (v * v).sum()
    col = lambda u: VB(u.v[:, None], u.b[:, None], u.m)
    row = lambda u: VB(u.v[None, :], u.b[None, :], u.m)
    M = VB(np.eye(len(v.v))) + 4.0 * vsq * (col(jv) * row(jv)) - 2.0 * (col(jv) * row(v) + col(v) * row(jv))
    return M / (beta * beta)


def pre_sums(t, th, z, x, X1, X2, wr, n):
    """what k_t3_pre adds to the partial sums of the stage: -> (theta'z + x's, |r_theta|^2 + r_t^2, m + 1)"""
    ta, tb, c, we = tri(n)
    s = slack(t, th, wr, n)
    x = VB.of(x)
    xs = x[0] * s[0] + dot1(x, s)
    r = -(VB(we) * (VB(X1)[ta, tb] - VB(X2)[ta, tb])) - VB(z) - VB(wr * c, m=1) * x[1:]
    rt = 1.0 - x[0]
    return (VB(th) * VB(z)).sum() + xs, (r * r).sum() + rt * rt, len(ta) + 1


# ---------------------------------------------------------------------------------------------------------------- k_t3_schur
def gram(L, R, ra, rb, ca, cb):
    """<E_ab, L E_cd R'> over rows (a, b) and columns (c, d): E_ab = e_a e_b' + e_b e_a' (a < b), e_a e_a' (a = b)"""
    L, R = VB.of(L), VB.of(R)
    a, b, c, d = ra[:, None], rb[:, None], ca[None, :], cb[None, :]
    t = (L[a, c] * R[b, d] + L[a, d] * R[b, c]) + (L[b, c] * R[a, d] + L[b, d] * R[a, c])
    return VB(np.where(a == b, 0.5, 1.0) * np.where(c == d, 0.5, 1.0)) * t


def schur_rows(X, Si, V, beta, v, th, z, wr, nx):
    """the rows of (theta_k, t_k) from X_r, S_r^-1 [2, n, n], V = [A B] [nx, n] and the scaling:
    -> dict(b [m, d] coupling with P_{k+1}, a [m, d] with P_k, H [m, m] theta-theta, trow [m + 1] the row of t over (theta, t))"""
    n = X.shape[-1]
    ta, tb, c, _ = tri(n)
    ia, ib = np.triu_indices(nx)
    m = len(ta)
    Vt = VB(V).T
    b = a = H = None
    for r in (0, 1):
        Xr, Sr = VB(X[r]), VB(Si[r])
        gb = gram(Xr @ Vt, Sr @ Vt, ta, tb, ia, ib)
        ga = gram(Xr, Sr, ta, tb, ia, ib)
        gh = gram(Xr, Sr, ta, tb, ta, tb)
        b, a, H = (gb, ga, gh) if r == 0 else (b + gb, a + ga, H + gh)
    W2 = w2inv(beta, v)
    wc = VB(wr * c, m=1)
    col = VB(wc.v[:, None], wc.b[:, None], 1); row = VB(wc.v[None, :], wc.b[None, :], 1)
    H = H + col * row * W2[1:, 1:]
    zt = VB(z) / VB(th)
    H = H + VB(np.diag(zt.v), np.diag(zt.b), zt.m)
    return dict(b=b, a=-a, H=H, trow=cat([wc * W2[0, 1:], W2[0, 0]]), m=m)


def cross(w, u, n):
    """the block between theta and the multipliers of G / C from the per-row vectors w = X_r g, u = S_r^-1 g [2, rows, n]: -> [m, rows]"""
    ta, tb, _, _ = tri(n)
    w, u = VB(w), VB(u)
    out = None
    for r in (0, 1):
        wa, wb_, ua, ub = w[r][:, ta], w[r][:, tb], u[r][:, ta], u[r][:, tb]
        t = where((ta == tb)[None, :], wa * ua, wa * ub + wb_ * ua)
        out = t if out is None else out + t
    return out.T


# ---------------------------------------------------------------------------------------------------------------- k_t3_rhs, k_t3_gather
def rhs_g(t, th, x, cq, sig, wr, n):
    """g = sig s^-1 - x - corr (cq None: no Mehrotra term)"""
    s = slack(t, th, wr, n)
    g = VB(sig) * J(s) / det(s) - VB(x)
    return g if cq is None else g - VB(cq)


def gather_rows(T1, T2, th, cth, g, x, Psi, Phi, sig, wr, n):
    """-> (r [m + 1] right-hand side of (theta, t), c_tau [m], c_alpha [m]); cth None: no Mehrotra term.  c_tau, c_alpha are exact (one product with 1 or 2)"""
    ta, tb, c, we = tri(n)
    g, x = VB(g), VB(x)
    r = VB(we) * (VB(T1)[ta, tb] - VB(T2)[ta, tb]) + VB(sig) / VB(th)
    if cth is not None:
        r = r - VB(cth)
    r = r + VB(wr * c, m=1) * (g[1:] + x[1:])
    return cat([r, (g[0] + x[0]) - 1.0]), -we * np.asarray(Psi)[ta, tb], we * np.asarray(Phi)[ta, tb]


# ---------------------------------------------------------------------------------------------------------------- k_t3_dir
def local_direction(Z, TU, dtau, dalpha):
    """the tail of the block solution: Z - TU[:, 0] dtau - TU[:, 1] dalpha"""
    TU = VB(TU)
    return VB(Z) - TU[:, 0] * VB(dtau) - TU[:, 1] * VB(dalpha)


def dual_direction(th, z, dth, sig, cth):
    th, z = VB(th), VB(z)
    dz = VB(sig) / th - z - z * VB(dth) / th
    return dz if cth is None else dz - VB(cth)


def mehrotra_theta(dz, dth, th):
    return VB(dz) * VB(dth) / VB(th)


def cone_ds(dt, dth, wr, n):
    _, _, c, _ = tri(n)
    return cat([VB(dt), VB(wr * c, m=1) * VB(dth)])


def cone_dx(g, beta, v, ds):
    """dx = g - W^-2 ds by the rank-two form"""
    beta, v, ds = VB.of(beta), VB.of(v), VB.of(ds)
    ib2 = 1.0 / (beta * beta)
    vsq = v[0] * v[0] + dot1(v, v)
    vu1 = dot1(v, ds)
    vu, jvu = v[0] * ds[0] + vu1, v[0] * ds[0] - vu1
    jv = J(v)
    return VB(g) - ib2 * (ds + 4.0 * vsq * jv * jvu - 2.0 * (jv * vu + v * jvu))


def jordan(u, w):
    u, w = VB.of(u), VB.of(w)
    return cat([(u * w).sum(), u[0] * w[1:] + w[0] * u[1:]])


def jordan_div(lam, r):
    """solve lam o u = r"""
    lam, r = VB.of(lam), VB.of(r)
    dl = det(lam)
    lr1 = dot1(lam, r)
    return cat([(lam[0] * r[0] - lr1) / dl, (-(r[0] * lam[1:]) + (dl * r[1:] + lr1 * lam[1:]) / lam[0]) / dl])


def W_apply(beta, v, u, inverse=False):
    beta, v, u = VB.of(beta), VB.of(v), VB.of(u)
    if inverse:
        jv = J(v)
        return (2.0 * jv * (jv * u).sum() - J(u)) / beta
    return beta * (2.0 * v * (v * u).sum() - J(u))


def cone_mehrotra(beta, v, lam, dx, ds):
    """corr = W^-1 (lambda \\ ((W dx) o (W^-1 ds)))"""
    return W_apply(beta, v, jordan_div(lam, jordan(W_apply(beta, v, dx), W_apply(beta, v, ds, inverse=True))), inverse=True)


# ---------------------------------------------------------------------------------------------------------------- k_t3_steps
def linear_steps(th, z, dth, dz):
    """the "eigenvalues" min(0, min dth / th), min(0, min dz / z) in fp64: a correctly rounded division and minima, bit-exact"""
    th, z, dth, dz = (np.asarray(a, float) for a in (th, z, dth, dz))
    return min(0.0, float(np.min(dth / th))), min(0.0, float(np.min(dz / z)))


def sums(th, z, dth, dz, s, ds, x, dx):
    """-> [<dx, s>, <x, ds>, <dx, ds>] over the linear cone and the norm cone"""
    f = lambda a, b, c, d: (VB(a) * VB(b)).sum() + (VB.of(c) * VB.of(d)).sum()
    return [f(dz, th, dx, s), f(z, dth, x, ds), f(dz, dth, dx, ds)]


def soc_poly(u, du):
    """det(u + th du) = c + 2 b th + a th^2 in longdouble"""
    u, du = np.asarray(u, LD), np.asarray(du, LD)
    return du[0] * du[0] - du[1:] @ du[1:], u[0] * du[0] - u[1:] @ du[1:], u[0] * u[0] - u[1:] @ u[1:]


def soc_inside(u, du, th):
    """u + th du strictly inside the cone (longdouble)"""
    w = np.asarray(u, LD) + LD(th) * np.asarray(du, LD)
    return bool(w[0] > 0 and w[0] * w[0] - w[1:] @ w[1:] > 0)


def soc_step_bisect(u, du):
    """largest th with u + th du in the cone, by bracketing: the cone is convex, so the set of feasible th >= 0 is an interval [0, th*]; np.inf exactly when du
    itself lies in the closed cone (u + th du is then a sum of cone points for every th)"""
    d = np.asarray(du, LD)
    if d[0] >= 0 and d[0] * d[0] - d[1:] @ d[1:] >= 0:
        return np.inf
    hi = LD(1)
    while soc_inside(u, du, hi):
        hi = hi * 2
        assert hi < 1e60, 'no exit from the cone found'
    lo = LD(0)
    for _ in range(300):
        mid = np.sqrt(lo * hi) if lo > 0 and hi / lo > 4 else 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if soc_inside(u, du, mid):
            lo = mid
        else:
            hi = mid
    return float(lo)


def soc_root_residual(u, du, th):
    """|det(u + th du)| / (|u0 + th du0|^2 + |u1 + th du1|^2) in longdouble: in units of eps, how far th is from a root of the boundary"""
    w = np.asarray(u, LD) + LD(th) * np.asarray(du, LD)
    return float(abs(w[0] * w[0] - w[1:] @ w[1:]) / (w[0] * w[0] + w[1:] @ w[1:]))


def soc_step_eig64(u, du):
    """fp64 numpy restatement of soc_step_eig (tmpc_t3.h), the same branches: the roots as q / a and c / q, q = -bq -+ sqrt(disc) without cancellation"""
    u, du = np.asarray(u, float), np.asarray(du, float)
    a = du[0] * du[0] - du[1:] @ du[1:]
    bq = u[0] * du[0] - u[1:] @ du[1:]
    c = u[0] * u[0] - u[1:] @ u[1:]
    th = 1e300
    if du[0] < 0.0:
        th = min(th, -u[0] / du[0])
    if abs(a) < 1e-300:
        if bq < 0.0:
            th = min(th, -c / (2.0 * bq))
    else:
        disc = bq * bq - a * c
        if disc >= 0.0:
            sq = np.sqrt(disc)
            q = (-bq + sq) if bq < 0.0 else (-bq - sq)
            for r in (q / a, c / q if q != 0.0 else -1.0):
                if r > 0.0:
                    th = min(th, r)
    return -1.0 / th if th < 1e299 else 0.0


# ---------------------------------------------------------------------------------------------------------------- k_t3_update
def update(x, dx, a):
    return VB(x) + VB(a) * VB(dx)
