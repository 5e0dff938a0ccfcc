"""The substitution sweeps of a float32 problem (k_cr_fwd_diag / k_cr_fwd_off / k_cr_bwd on the float32 copies of the O blocks, wg_gemv32f of
tmpc_factor.h: 64 x 32 slabs) against their specification (GPU tests: -m gpu on an MI355X; the check of the specification itself runs anywhere).

Specification: with the images the call itself returns -- L (lower triangle of oD), the float32 O factors of every edge and fill slot (oO32), the
schedule and its orientation -- the level-by-level substitution  z_i <- L_i^-1 z_i,  z_s -= O_s z_i  and back  z_i <- L_i^-T (z_i - O_a' z_a - O_b' z_b),
in numpy: once in fp64 and once in longdouble with O32 widened.  It does not depend on the slab geometry of the kernel nor on the rounding of the
factorisation (the factor is an input).  Asserted: the error of the GPU's X against the longdouble walk is at most 4 x the error of the fp64 walk
against it (the margin of tests/test_gpu_factor_kernels.py for reference-relative bounds: the orders of summation differ, and the kernel multiplies
by inverted 64 x 64 diagonal tiles where numpy substitutes), plus a floor of 4 u ||x||_2, u = 2^-53 (a correctly rounded x is already off by up to
u ||x||; where the fp64 walk happens to land within an ulp or two of the longdouble one, 4 x its error asks for less than fp64 can hold).

Shapes: the float32 path exists for 64 < dp <= 320; d = dp in {80, 96, 112, 128, 144, 160} with p = 2, 3 reach every boundary of the 32-deep loop
(2 .. 5 full slabs, with and without the half-slab tail, one or two full 64-row blocks with partial ones of 16 / 32 / 48 rows, all four prefetch sets
with and without a refill), d = 300 (dp = 304 = 9 x 32 + 16, ld32 = 320, real padding) is the flagship block.  cond(T) ~ 1e3 throughout.

Figures on an MI355X, per shape over pass 2 / pass 1 / fused, every right-hand side and both policies (the FIG lines the tests print):
      d  p   err(GPU) / bound asserted   err(GPU) / err(fp64 walk)   err(GPU) / ||x||
     80  2   <= 0.328                    1.05 ... 1.70               <= 6.5e-16
     80  3   <= 0.394                    1.09 ... 2.09               <= 7.2e-16
     96  2   <= 0.342                    0.92 ... 1.82               <= 6.4e-16
     96  3   <= 0.320                    1.04 ... 1.64               <= 6.8e-16
    112  2   <= 0.434                    1.12 ... 2.16               <= 9.8e-16
    112  3   <= 0.321                    1.08 ... 1.63               <= 6.9e-16
    128  2   <= 0.461                    1.07 ... 2.45               <= 8.2e-16
    128  3   <= 0.338                    1.12 ... 1.68               <= 8.8e-16
    144  2   <= 0.366                    0.90 ... 1.83               <= 8.0e-16
    144  3   <= 0.365                    1.10 ... 1.80               <= 8.9e-16
    160  2   <= 0.355                    1.18 ... 1.80               <= 8.1e-16
    160  3   <= 0.347                    1.14 ... 1.73               <= 9.7e-16
    300  3   <= 0.392                    0.96 ... 1.86               <= 1.1e-15
  The 4 x margin alone (no floor) holds everywhere: the GPU is within 2.45 x the fp64 walk.  The module takes 5 s of the GPU suite's wall time.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch ships its own HIP runtime and fails to find the GPU when it initialises second)

import cr_reference as cr  # noqa: E402

U64 = 2.0 ** -53
COND = 1e3
SHAPES = [(p, d) for d in (80, 96, 112, 128, 144, 160) for p in (2, 3)] + [(3, 300)]
POLICIES = {'f32_updates': False, 'f32_trsm': True}       # policy -> DF_LOWP_TRSM (I_LOWP is set in both)
KINDS = ('pass2', 'pass1', 'fused')


# ----------------------------------------------------------------------------- the specification
def _tri_solve(L, z, trans, dtype):
    """L^-1 z (trans: L^-T z) by substitution, every operation in `dtype`; z [d, nc]"""
    d = L.shape[0]
    L = L.astype(dtype); z = z.astype(dtype).copy()
    if not trans:
        for i in range(d):
            z[i] = (z[i] - L[i, :i] @ z[:i]) / L[i, i]
    else:
        for i in range(d - 1, -1, -1):
            z[i] = (z[i] - L[i + 1:, i] @ z[i + 1:]) / L[i, i]
    return z


def substitute(sched, L, O, rhs, dtype):
    """forward and backward substitution along the schedule with the factor given: L {node: L_i} or [p, d, d], O {slot: block} or [2p, d, d] (O factors of
    the edge and fill slots in the slot orientation), rhs [p, d] or [p, d, nc].  Every operation in `dtype`.  Returns x in the shape of rhs."""
    z = np.asarray(rhs, dtype)
    z = z.reshape(z.shape[0], z.shape[1], -1).copy()
    Ow = lambda e: np.asarray(O[e], dtype)
    for (eoff, nelim, uoff, nupd) in sched['levels']:
        for r in sched['elim'][eoff:eoff + nelim]:
            z[r[0]] = _tri_solve(L[r[0]], z[r[0]], False, dtype)
        for u in sched['upd'][uoff:uoff + nupd]:
            for e, src in ((u[1], u[2]), (u[3], u[4])):
                if e >= 0:
                    z[u[0]] = z[u[0]] - Ow(e) @ z[src]
    for (eoff, nelim, uoff, nupd) in sched['levels'][::-1]:
        for r in sched['elim'][eoff:eoff + nelim]:
            for e, nb in ((r[3], r[1]), (r[4], r[2])):
                if e >= 0:
                    z[r[0]] = z[r[0]] - Ow(e).T @ z[nb]
            z[r[0]] = _tri_solve(L[r[0]], z[r[0]], True, dtype)
    return z.reshape(np.shape(rhs))


def _sched(p):
    from tunempc_amd._lib import cr_schedule
    return cr_schedule(p)


@pytest.mark.parametrize('p,d', [(3, 80), (5, 112)])
def test_specification_solves_the_system(p, d):
    """the numpy substitution on the factor of the fp64 reference factorisation (tests/cr_reference.py) solves T x = b as numpy.linalg.solve does:
    both within cond(T) x 8 u of each other (two backward-stable fp64 solves), in fp64 and in longdouble arithmetic, one and three right-hand sides"""
    c = cr.case(p, d, COND)
    sched = _sched(p)
    T = cr.dense(c['D'][0], c['Cc'][0])
    for rhs in (c['b1'][0], c['b3'][0]):
        r = cr.reference(sched, c['D'][0], c['Cc'][0], rhs, 'fp64')
        xs = np.linalg.solve(T, rhs.reshape(p * d, -1)).reshape(rhs.shape)
        for dtype in (np.float64, np.longdouble):
            x = substitute(sched, r['L'], r['slots'], rhs, dtype)
            assert x.shape == rhs.shape and x.dtype == dtype
            assert cr.rel(x.astype(np.float64), xs) <= 8 * U64 * c['cond'][0]
        assert cr.rel(substitute(sched, r['L'], r['slots'], rhs, np.float64), r['x']) <= 8 * U64 * c['cond'][0]


# ----------------------------------------------------------------------------- the kernels
@pytest.fixture(scope='module')
def h():
    from tunempc_amd._lib import HipConvexifier
    hh = HipConvexifier(2, 3, 1)
    yield hh
    hh.close()


def _run(h, c, rhs, kind, trsm, **kw):
    return h.debug_block_factor(c['D'], c['Cc'], rhs, lowp_trsm=trsm, pass1=kind != 'pass2', fuse_fwd1=kind == 'fused', **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('policy', list(POLICIES))
@pytest.mark.parametrize('p,d', SHAPES)
def test_substitution_against_the_read_back_images(h, p, d, policy):
    c = cr.case(p, d, COND)
    sched = _sched(p)
    worst = 0.0
    spec = {}
    for kind in KINDS:
        rhs = c['b1'] if kind == 'pass2' else c['b3']
        g = _run(h, c, rhs, kind, POLICIES[policy], lowp=[1])
        assert g['nshift'][0] == 0 and np.array_equal(g['orient'], sched['orient'])
        raw = g['raw']
        dp, ld32 = raw['dp'], raw['ld32']
        assert raw['O32'].shape == (1, 2 * p, dp, ld32) and raw['X'].shape[:3] == (1, p, dp)
        # padding: rows d .. dp of X, rows d .. dp and columns d .. ld32 of every float32 block
        assert np.all(raw['X'][:, :, d:] == 0.0)
        assert np.all(raw['O32'][:, :, d:, :] == 0.0) and np.all(raw['O32'][:, :, :, d:] == 0.0)
        # the factor is the same in every kind (the fused sweep changes where the forward step runs, not the factor): one specification per kind of right-hand side
        key = kind == 'pass2'
        if key not in spec:
            spec[key] = (g['L'][0].copy(), g['O32'][0].copy(),
                         substitute(sched, g['L'][0], g['O32'][0], rhs[0], np.longdouble), substitute(sched, g['L'][0], g['O32'][0], rhs[0], np.float64))
        Ls, Os, xl, x64 = spec[key]
        assert np.array_equal(g['L'][0], Ls) and np.array_equal(g['O32'][0], Os)
        xg = g['x'][0].reshape(p, d, -1); xl = xl.reshape(p, d, -1); x64 = x64.reshape(p, d, -1)
        for q in range(xg.shape[2]):
            nrm = float(np.linalg.norm(xl[..., q].astype(np.float64)))
            eg = float(np.linalg.norm((xg[..., q] - xl[..., q]).astype(np.float64)))
            er = float(np.linalg.norm((x64[..., q] - xl[..., q]).astype(np.float64)))
            bound = 4 * er + 4 * U64 * nrm
            print(f'FIG subst {policy} {kind} p{p} d{d} rhs{q}: gpu {eg:.3e} fp64-walk {er:.3e} |x| {nrm:.3e} gpu/bound {eg / bound:.3f} gpu/walk {eg / max(er, 1e-300):.2f}')
            worst = max(worst, eg / bound)
    print(f'FIG subst worst {policy} p{p} d{d}: {worst:.3f}')
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize('trsm', [False, True])
@pytest.mark.parametrize('kind', ['pass2', 'pass1', 'fused'])
@pytest.mark.parametrize('p,d', [(3, 80), (3, 300)])
def test_no_reads_behind_the_data(h, p, d, kind, trsm):
    """a float32 problem alone and the same problem listed among six distinct systems (float32 and fp64 neighbours before and behind it in memory): bit-equal X.
    A tail step that read the k rows behind the last float32 block of the problem (the next problem's) or multiplied by the LDS behind the vector would differ."""
    c = cr.case(p, d, COND, nb=6)
    rhs = c['b1'] if kind == 'pass2' else c['b3']
    plist = [4, 1, 2, 5]; lowp = np.array([0, 1, 1, 0, 0, 1], np.int32)
    mixed = _run(h, c, rhs, kind, trsm, plist=plist, lowp=lowp)
    assert not mixed['nshift'].any()
    for b in (1, 2, 5):
        alone = _run(h, dict(D=c['D'][b:b + 1], Cc=c['Cc'][b:b + 1]), rhs[b:b + 1], kind, trsm, lowp=[1])
        assert np.any(alone['raw']['O32'] != 0.0)
        assert np.array_equal(mixed['raw']['X'][b], alone['raw']['X'][0]), b
        assert np.array_equal(mixed['raw']['O32'][b], alone['raw']['O32'][0]), b
    assert np.all(mixed['raw']['X'][:, :, d:] == 0.0)
    assert np.all(mixed['raw']['O32'][:, :, d:, :] == 0.0) and np.all(mixed['raw']['O32'][:, :, :, d:] == 0.0)
