"""Kernel-level tests of the block factorisation in its three fp64 / float32 precisions and in double-double (run with -m gpu on an MI355X).

The end-to-end parity tests cannot see a wrong linear solve: the interior-point iteration ends with Newton centering whose residuals are recomputed
from the iterate, so a factorisation that is less accurate than it should be only changes the road.  Here the factorisation is driven as the solver
drives it (tmpc_debug_block_factor: problem list, per-problem I_LOWP, DF_LOWP_TRSM, pass, fused forward sweep) and its factor and solutions are
compared with tests/cr_reference.py, the numpy walk of the library's own schedule under the same precision policy, and with a longdouble / exact-residual truth.

How the bounds are fixed -- from the CPU reference on the very input of the test (computed in the test), never from the GPU's output:
  * backward errors  ||T x - b||_2 / (||T||_2 ||x||_2 + ||b||_2)  (longdouble) and the element-level residual of the float32 solves:
    4 x the same quantity of the reference under the same policy (||T||_2, not the Frobenius norm: cond_2(T) times it bounds the forward error);
  * double-double: ||b - T (hi + lo)||_2 / (||T||_2 ||x||_2) <= 4 u_dd, u_dd = 2^-104 = 4.9e-32 the unit roundoff of the double-word operations tmpc_dd.h
    is built from (Dekker product with the cross terms rounded once, accumulators whose low word collects in fp64 until the tile is stored: relative
    error 3 ... 7 x 2^-106 per operation -- Joldes, Muller, Popescu, ACM TOMS 44 (2017)).  This is the rule above in the form it takes when the
    reference is not written in the arithmetic of the kernel: a backward-stable solve sits at about one unit roundoff of its format (the fp64 reference
    measures 0.3 ... 1.3 u, the float32 ones 0.2 ... 0.9 u), so 4 x reference = 4 u.  The numpy double-double walk (cr_reference.reference_dd on
    oracle/ddnum.py) renormalises after every operation and sums with the accurate double-word addition: it measures 0.02 ... 0.16 u_dd, the kernels
    0.08 ... 0.82 u_dd on the same inputs at every cond(T) alike.  4 x THAT reference was the first choice here and the kernels miss it by up to 2.3 x (they sit at up to 9.4 x the reference):
    two correct double-word arithmetics with different error constants, not a defect.  The reference figure is printed beside every dd assertion;
  * block distances (relative Frobenius, per block): fp64 against the fp64 reference: 8 u cond(T), u = 2^-53 -- two backward-stable fp64
    factorisations of one matrix differ by their backward errors (a few u) times the sensitivity of the factor, which cond(T) bounds (Sun 1991);
    float32 policies against the FP64 reference: 8 x the distance of the numpy float32 reference to the fp64 reference on the same input, plus the
    fp64 term (the first-level L of a float32 problem is an fp64 Cholesky: its reference distance is zero);
  * forward errors: cond(T) x the backward bound; fused against unfused forward sweep: bit-equal for float32 problems (both run k_cr_fwd_diag /
    k_cr_fwd_off), 2 cond(T) x the backward bound in fp64 (the fused step sums inside the MFMA tile);
  * margin 4 / 8: the reference accumulates a float32 dot product in OpenBLAS order, the MFMA tile in 4-wide K steps over 64-wide slabs; both obey the
    same gamma_k bound, and the inverted 64 x 64 diagonal tiles add a factor of the tile's condition number that back substitution does not have.
Conditions: nshift == 0 on every input (tests/test_cr_reference.py: every policy factors every case on the CPU without a non-positive pivot).

Figures (reference value / MI355X value / bound asserted), ranges over the cases of cr_reference.F32_CASES / FP64_CASES / DD_CASES:
  quantity (policy)                                        reference             MI355X                bound asserted
  (a) ||O32 L' - E|| / (||O32|| ||L||), first level
        f32_updates (float32 store of k_cr_trsm_dma)       1.4e-9 ... 3.2e-9     1.4e-9 ... 3.2e-9     4 x reference (MI355X / reference <= 1.00)
        f32_trsm    (k_cr_trsm_dma_f32)                    7.2e-9 ... 1.8e-8     1.0e-8 ... 1.8e-8     4 x reference (<= 2.20)
  (b) distance of a block to the fp64 reference block
        fp64         L_i / O, F slots                      --                    1e-16 ... 6e-11       8 u cond(T) = 2e-14 ... 5e-8 (MI355X / bound <= 0.13)
        f32_updates  L_i / O32 slots                       0 ... 5.7e-5 / 8e-6   2e-16 ... 5.8e-5 / 8e-6   8 x reference + 8 u cond(T) (<= 0.20)
        f32_trsm     L_i / O32 slots / E in the fp64 slots 0 ... 7.2e-5 / 1.3e-5 / 4.7e-6   ... 6.5e-5 / 1.2e-5 / 4.2e-6   the same (<= 0.27)
  (c) backward error of a solve (pass 2, pass 1 x 3, fused)
        fp64 (all kernel families, cond(T) 2e1 ... 5e7)    3.0e-17 ... 1.4e-16   2.2e-17 ... 2.0e-16   4 x reference (MI355X / reference <= 2.31)
        f32_updates                                        1.2e-8 ... 4.2e-8     1.2e-8 ... 4.1e-8     4 x reference (<= 1.56)
        f32_trsm                                           2.0e-8 ... 5.1e-8     1.6e-8 ... 5.7e-8     4 x reference (<= 1.63)
      forward error / (cond(T) x backward bound)           --                    <= 0.16               1
  (f) double-double residual, cond(T) 6e3 ... 3e11         0.9e-33 ... 7.8e-33   4.2e-33 ... 4.0e-32   4 x 2^-104 = 2.0e-31 (MI355X / reference <= 9.4)
      forward error against mpmath, cond(T) 2.6e11         --                    1.1e-22               cond(T) x 2.0e-31 = 5.1e-20
  The module takes 34 s of the GPU suite's wall time.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch ships its own HIP runtime and fails to find the GPU when it initialises second)

pytestmark = pytest.mark.gpu

import cr_reference as cr  # noqa: E402

U64 = 2.0 ** -53
UDD = 2.0 ** -104       # unit roundoff of the double-word operations of tmpc_dd.h (see the module docstring)
FLAG_NO_MFMA, FLAG_NO_DMA = 1, 32
MODES = {'fp64': (0, False), 'f32_updates': (1, False), 'f32_trsm': (1, True)}      # policy -> (I_LOWP, DF_LOWP_TRSM)
FLOAT_PARAMS = [(p, d, c, pol) for (p, d, c) in cr.F32_CASES for pol in ('f32_updates', 'f32_trsm')]
ALL_PARAMS = [(p, d, c, pol) for (p, d, c) in cr.F32_CASES for pol in cr.POLICIES] + [(p, d, c, 'fp64') for (p, d, c) in cr.FP64_CASES]


@pytest.fixture(scope='module')
def h():
    from tunempc_amd._lib import HipConvexifier
    hh = HipConvexifier(2, 3, 1)
    yield hh
    hh.close()


def _sched(p):
    from tunempc_amd._lib import cr_schedule
    return cr_schedule(p)


_GPU, _REF, _TRUTH = {}, {}, {}


def gpu(h, p, d, cond, policy, kind, flags=0):
    """one problem through the kernels; kind: 'pass2' (one right-hand side in Z), 'pass1' (three in W3), 'fused' (pass 1, forward sweep inside the factorisation)"""
    key = (p, d, cond, policy, kind, flags)
    if key not in _GPU:
        c = cr.case(p, d, cond)
        lowp, trsm = MODES[policy]
        h.set_options(flags=flags)
        try:
            _GPU[key] = h.debug_block_factor(c['D'], c['Cc'], c['b1'] if kind == 'pass2' else c['b3'], lowp=[1] if lowp else None, lowp_trsm=trsm,
                                             pass1=kind != 'pass2', fuse_fwd1=kind == 'fused')
        finally:
            h.set_options(flags=0)
    return _GPU[key]


def ref(p, d, cond, policy, kind='pass2'):
    key = (p, d, cond, policy, kind != 'pass2')
    if key not in _REF:
        c = cr.case(p, d, cond)
        _REF[key] = cr.reference(_sched(p), c['D'][0], c['Cc'][0], c['b1'][0] if kind == 'pass2' else c['b3'][0], policy)
    return _REF[key]


def truth(p, d, cond):
    """(longdouble dense T, longdouble solutions of [b1 | b3])"""
    key = (p, d, cond)
    if key not in _TRUTH:
        c = cr.case(p, d, cond)
        Tl = cr.dense(c['D'][0], c['Cc'][0], np.longdouble)
        B = np.concatenate([c['b1'][0].reshape(p * d, 1), c['b3'][0].reshape(p * d, 3)], axis=1)
        _TRUTH[key] = (Tl, cr.solve_truth(Tl, B))
    return _TRUTH[key]


def check(what, got, bound, ref_value=None):
    """print the figure, then assert it (the job that measured the table of the docstring kept this output)"""
    print(f'FIG {what}: gpu {got:.3e} bound {bound:.3e}' + ('' if ref_value is None else f' ref {ref_value:.3e}'))
    assert got <= bound, (what, got, bound)


def fused_ok(p, d):
    dp = (d + 15) // 16 * 16
    return p > 1 and 16 < dp <= 320


# ----------------------------------------------------------------------------- (a) the float32 solve, element level
@pytest.mark.parametrize('p,d,cond,policy', FLOAT_PARAMS)
def test_first_level_float32_solve(h, p, d, cond, policy):
    """First level: E is the given coupling block, L the Cholesky factor of the given D_i (compared with numpy first), so the inputs of k_cr_trsm_dma_f32
    (f32_trsm) / of the float32 store of k_cr_trsm_dma (f32_updates) are known exactly: ||O32 L' - E||_F / (||O32||_F ||L||_F) against the same quantity of
    the reference; and the padding of O32 (rows / columns d .. ld32) is exactly zero after the call."""
    c = cr.case(p, d, cond)
    g = gpu(h, p, d, cond, policy, 'pass2'); r = ref(p, d, cond, policy)
    assert g['nshift'][0] == 0
    sched = _sched(p)
    eoff, nelim = sched['levels'][0][:2]
    for rec in sched['elim'][eoff:eoff + nelim]:
        node = int(rec[0])
        Ln = np.linalg.cholesky(c['D'][0, node]); Lg = g['L'][0, node]
        check(f'a L p{p} d{d} node{node}', cr.rel(Lg, Ln), 8 * U64 * np.linalg.cond(c['D'][0, node]))
        for e in (int(rec[3]), int(rec[4])):
            if e < 0:
                continue
            E = r['pre'][e]
            qr = cr.block_trsm_residual(r['slots'][e], r['L'][node], E)
            qg = cr.block_trsm_residual(g['O32'][0, e], Lg, E)
            check(f'a trsm {policy} p{p} d{d} slot{e}', qg, 4 * qr, qr)
    raw = g['raw']['O32']
    assert raw.shape == (1, 2 * p, g['raw']['dp'], g['raw']['ld32'])
    assert np.all(raw[:, :, d:, :] == 0.0) and np.all(raw[:, :, :, d:] == 0.0)


# ----------------------------------------------------------------------------- (b) the whole factor, block by block
@pytest.mark.parametrize('p,d,cond,policy', ALL_PARAMS)
def test_factor_blocks(h, p, d, cond, policy):
    """every L_i and every edge / fill slot against the schedule-walking reference (bounds: module docstring)"""
    c = cr.case(p, d, cond)
    g = gpu(h, p, d, cond, policy, 'pass2'); r = ref(p, d, cond, policy); r64 = ref(p, d, cond, 'fp64')
    assert g['nshift'][0] == 0
    b64 = 8 * U64 * c['cond'][0]
    flt = policy != 'fp64'
    worst = [0.0, 0.0]
    for i in range(p):
        dref = cr.rel(r['L'][i], r64['L'][i])
        dg = cr.rel(g['L'][0, i], r64['L'][i])
        print(f'FIG b L {policy} p{p} d{d} node{i}: gpu {dg:.3e} ref {dref:.3e} bound {8 * dref + b64:.3e}')
        worst[0] = max(worst[0], dg / (8 * dref + b64))
    slot64 = lambda o, e: (o['O'] if e < p else o['F'])[0, e % p]
    for e in sorted(r64['solved']):
        dref = cr.rel(r['slots'][e], r64['slots'][e])
        dg = cr.rel(g['O32'][0, e] if flt else slot64(g, e), r64['slots'][e])
        print(f'FIG b O {policy} p{p} d{d} slot{e}: gpu {dg:.3e} ref {dref:.3e} bound {8 * dref + b64:.3e}')
        worst[1] = max(worst[1], dg / (8 * dref + b64))
        if policy == 'f32_trsm':            # the fp64 slot of such a problem is never solved: it still holds E, with every float32 update of the levels before in it
            dref = cr.rel(r['pre'][e], r64['pre'][e]); dg = cr.rel(slot64(g, e), r64['pre'][e])
            print(f'FIG b E {policy} p{p} d{d} slot{e}: gpu {dg:.3e} ref {dref:.3e} bound {8 * dref + b64:.3e}')
            worst[1] = max(worst[1], dg / (8 * dref + b64))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


# ----------------------------------------------------------------------------- (c) solves
def _solve_checks(h, p, d, cond, policy, flags=0):
    c = cr.case(p, d, cond)
    Tl, xt = truth(p, d, cond)
    kinds = ['pass2', 'pass1'] + (['fused'] if fused_ok(p, d) and not flags else [])
    xs = {}
    be_bound = 0.0
    for kind in kinds:
        g = gpu(h, p, d, cond, policy, kind, flags)
        assert g['nshift'][0] == 0
        r = ref(p, d, cond, policy, kind)
        cols = [(g['x'][0], r['x'], c['b1'][0], xt[:, 0])] if kind == 'pass2' else [(g['x'][0][..., q], r['x'][..., q], c['b3'][0][..., q], xt[:, 1 + q]) for q in range(3)]
        for q, (xg, xr, b, x_true) in enumerate(cols):
            be_r = cr.backward_error(Tl, xr, b, c['norm2'][0])
            be_bound = max(be_bound, 4 * be_r)
            check(f'c backward {policy} {kind} p{p} d{d} flags{flags} rhs{q}', cr.backward_error(Tl, xg, b, c['norm2'][0]), 4 * be_r, be_r)
            check(f'c forward {policy} {kind} p{p} d{d} flags{flags} rhs{q}', cr.rel(xg.ravel(), x_true.astype(np.float64)), c['cond'][0] * 4 * be_r)
        xs[kind] = g['x'][0]
    if 'fused' in xs:
        if policy == 'fp64':
            check(f'c fused-vs-unfused {policy} p{p} d{d}', cr.rel(xs['fused'], xs['pass1']), 2 * c['cond'][0] * be_bound)
        else:
            assert np.array_equal(xs['fused'], xs['pass1'])


@pytest.mark.parametrize('p,d,cond,policy', ALL_PARAMS)
def test_solves(h, p, d, cond, policy):
    """normwise backward error (longdouble) of pass 2 and of each right-hand side of pass 1, fused and unfused forward sweep, and the forward error"""
    _solve_checks(h, p, d, cond, policy)


@pytest.mark.parametrize('flags', [FLAG_NO_DMA, FLAG_NO_MFMA])
@pytest.mark.parametrize('p,d,cond', [(3, 129, 1e2), (4, 144, 1e5), (4, 40, 1e5), (2, 65, 1e8)])
def test_register_staged_and_scalar_paths(h, p, d, cond, flags):
    """k_cr_potrf / k_cr_trsm / k_cr_update (the path of blocks wider than 320) at small shapes, and their scalar-FMA twins: same assertions"""
    _solve_checks(h, p, d, cond, 'fp64', flags)
    g = gpu(h, p, d, cond, 'fp64', 'pass2', flags); r64 = ref(p, d, cond, 'fp64')
    b64 = 8 * U64 * cr.case(p, d, cond)['cond'][0]
    for i in range(p):
        check(f'b L fp64 flags{flags} p{p} d{d} node{i}', cr.rel(g['L'][0, i], r64['L'][i]), b64)


# ----------------------------------------------------------------------------- (d) not vacuous
@pytest.mark.parametrize('p,d,cond', cr.F32_CASES)
def test_float32_kernels_ran(h, p, d, cond):
    """a float32 policy whose solution equals the fp64 one, or float32 solves whose O32 equals the rounded fp64 solves bit for bit, did not run the kernel under test"""
    x64 = gpu(h, p, d, cond, 'fp64', 'pass2')['x']
    gu = gpu(h, p, d, cond, 'f32_updates', 'pass2'); gt = gpu(h, p, d, cond, 'f32_trsm', 'pass2')
    assert cr.rel(gu['x'], x64) > 1e-10 and cr.rel(gt['x'], x64) > 1e-10
    assert not np.array_equal(gu['O32'], gt['O32'])
    assert np.any(gu['O32'] != 0.0) and np.any(gt['O32'] != 0.0)


# ----------------------------------------------------------------------------- (e) lists and mixed batches
RAW_KEYS = ('D', 'O', 'F', 'Ddiag', 'X', 'O32')


def _same(a, b):
    """bit-equal images; a call without a float32 problem has no O32: the other side's must then be untouched (all zero)"""
    return bool(np.all(a == 0.0)) if b is None else np.array_equal(a, b)


@pytest.mark.parametrize('trsm', [False, True])
@pytest.mark.parametrize('kind', ['pass2', 'fused'])
@pytest.mark.parametrize('p,d,cond', cr.LIST_CASES)
def test_lists_and_mixed_batches(h, p, d, cond, kind, trsm):
    """six distinct systems, the list [4, 1, 5] with problem 4 in fp64 and 1, 5 with float32 updates (trsm: and float32 solves); problem 2 is marked float32 but not listed"""
    c = cr.case(p, d, cond, nb=6)
    rhs = c['b1'] if kind == 'pass2' else c['b3']
    kw = dict(pass1=kind != 'pass2', fuse_fwd1=kind == 'fused', lowp_trsm=trsm)
    plist = [4, 1, 5]; lowp = np.array([0, 1, 1, 0, 0, 1], np.int32)
    mixed = h.debug_block_factor(c['D'], c['Cc'], rhs, plist=plist, lowp=lowp, **kw)
    assert not mixed['nshift'].any()
    assert np.array_equal(mixed['orient'], _sched(p)['orient'])
    # (ii) every array of every unlisted problem is what was uploaded (a call with an empty list runs no kernel: its read-back is the upload)
    up = h.debug_block_factor(c['D'], c['Cc'], rhs, plist=[], lowp=lowp, **kw)
    assert np.array_equal(up['D'], c['D']) and np.all(up['raw']['O32'] == 0.0)
    for b in (0, 2, 3):
        for k in RAW_KEYS:
            assert np.array_equal(mixed['raw'][k][b], up['raw'][k][b]), (b, k)
    for b in plist:
        assert not np.array_equal(mixed['raw']['D'][b], up['raw']['D'][b])
    # (i) each listed problem equals the same problem alone, in the same mode, bit for bit (the kernels claim that a problem's result does not depend on the batch)
    for b in plist:
        alone = h.debug_block_factor(c['D'][b:b + 1], c['Cc'][b:b + 1], rhs[b:b + 1], lowp=lowp[b:b + 1], **kw)
        for k in RAW_KEYS:
            assert _same(mixed['raw'][k][b], None if alone['raw'][k] is None else alone['raw'][k][0]), (b, k)
    # (iii) the fp64 problem of the mixed launch is bit-identical to an all-fp64 launch of the same list
    allf = h.debug_block_factor(c['D'], c['Cc'], rhs, plist=plist, pass1=kw['pass1'], fuse_fwd1=kw['fuse_fwd1'])
    for k in RAW_KEYS[:-1]:
        assert np.array_equal(mixed['raw'][k][4], allf['raw'][k][4]), k
    # ... and the float32 problems are not: their kernels ran
    assert not np.array_equal(mixed['raw']['X'][1], allf['raw']['X'][1]) and np.any(mixed['raw']['O32'][5] != 0.0)
    # the order of the list is immaterial
    perm = h.debug_block_factor(c['D'], c['Cc'], rhs, plist=[5, 4, 1], lowp=lowp, **kw)
    for k in RAW_KEYS:
        assert np.array_equal(mixed['raw'][k], perm['raw'][k]), k
    # and the listed problems are right, not only reproducible
    for b, pol in ((4, 'fp64'), (1, 'f32_trsm' if trsm else 'f32_updates')):
        r = cr.reference(_sched(p), c['D'][b], c['Cc'][b], rhs[b], pol)
        Tl = cr.dense(c['D'][b], c['Cc'][b], np.longdouble)
        for q in range(1 if kind == 'pass2' else 3):
            xg, xr, bb = (mixed['x'][b], r['x'], rhs[b]) if kind == 'pass2' else (mixed['x'][b][..., q], r['x'][..., q], rhs[b][..., q])
            be_r = cr.backward_error(Tl, xr, bb, c['norm2'][b])
            check(f'e backward {pol} {kind} p{p} d{d} problem{b} rhs{q}', cr.backward_error(Tl, xg, bb, c['norm2'][b]), 4 * be_r, be_r)


def test_lists_on_the_register_staged_kernels(h):
    """the same list handling on k_cr_potrf / k_cr_trsm / k_cr_update (TMPC_DEBUG_FLAG_NO_DMA; fp64 only: the float32 kernels are LDS-DMA kernels)"""
    p, d, cond = cr.LIST_CASES[0]
    c = cr.case(p, d, cond, nb=6)
    keys = RAW_KEYS[:-1]
    h.set_options(flags=FLAG_NO_DMA)
    try:
        out = h.debug_block_factor(c['D'], c['Cc'], c['b3'], plist=[4, 1, 5], pass1=True)
        up = h.debug_block_factor(c['D'], c['Cc'], c['b3'], plist=[], pass1=True)
        alone = {b: h.debug_block_factor(c['D'][b:b + 1], c['Cc'][b:b + 1], c['b3'][b:b + 1], pass1=True) for b in (4, 1, 5)}
        with pytest.raises(RuntimeError):      # no float32 path and no fused sweep on these kernels: refused, not rerouted
            h.debug_block_factor(c['D'], c['Cc'], c['b3'], lowp=np.ones(6, np.int32), pass1=True)
        with pytest.raises(RuntimeError):
            h.debug_block_factor(c['D'], c['Cc'], c['b3'], pass1=True, fuse_fwd1=True)
    finally:
        h.set_options(flags=0)
    assert not out['nshift'].any()
    for b in (0, 2, 3):
        for k in keys:
            assert np.array_equal(out['raw'][k][b], up['raw'][k][b]), (b, k)
    for b in (4, 1, 5):
        for k in keys:
            assert np.array_equal(out['raw'][k][b], alone[b]['raw'][k][0]), (b, k)
    dma = h.debug_block_factor(c['D'], c['Cc'], c['b3'], plist=[4, 1, 5], pass1=True)
    assert not np.array_equal(out['raw']['D'][4], dma['raw']['D'][4])      # (another kernel family ran: same factor to rounding, not bit for bit)
    assert cr.rel(out['L'][4], dma['L'][4]) < 8 * U64 * c['cond'][4]


# ----------------------------------------------------------------------------- (f) double-double
def _dd_quotient(D, Cc, xh, xl, b, Dlo=None, Clo=None):
    res = cr.dd_residual(D, Cc, xh, xl, b, Dlo, Clo)
    return float(np.linalg.norm(res) / (np.linalg.norm(cr.dense(D, Cc), 2) * np.linalg.norm(xh)))


@pytest.mark.parametrize('p,d,cond', cr.DD_CASES)
def test_dd_residual(h, p, d, cond):
    """||b - T (hi + lo)|| / (||T|| ||x||), every row of the residual correctly rounded (cr_reference.dd_residual), against 4 x the unit roundoff 2^-104 of the
    double-word operations (module docstring; the numpy double-double walk of the schedule is printed beside it); pass 2 everywhere, pass 1 (three right-hand sides) up to d = 136.  A solution that lost its low words
    sits at ~1e-17, sixteen orders above."""
    c = cr.case(p, d, cond)
    D, Cc = c['D'][0], c['Cc'][0]
    g = h.debug_block_factor(c['D'], c['Cc'], c['b1'], dd=True)
    assert g['nshift'][0] == 0
    r = cr.reference_dd(_sched(p), D, Cc, c['b1'][0])
    qr = _dd_quotient(D, Cc, r['xh'], r['xl'], c['b1'][0])
    check(f'f dd residual pass2 p{p} d{d} cond {c["cond"][0]:.1e}', _dd_quotient(D, Cc, g['x'][0], g['xl'][0], c['b1'][0]), 4 * UDD, qr)
    assert _dd_quotient(D, Cc, g['x'][0], np.zeros_like(g['xl'][0]), c['b1'][0]) > 1e6 * 4 * UDD       # (the low words carry the claim)
    if d <= 136:
        g3 = h.debug_block_factor(c['D'], c['Cc'], c['b3'], dd=True, pass1=True)
        r3 = cr.reference_dd(_sched(p), D, Cc, c['b3'][0])
        assert g3['nshift'][0] == 0
        for q in range(3):
            qr = _dd_quotient(D, Cc, r3['xh'][..., q], r3['xl'][..., q], c['b3'][0][..., q])
            check(f'f dd residual pass1 p{p} d{d} rhs{q}', _dd_quotient(D, Cc, g3['x'][0][..., q], g3['xl'][0][..., q], c['b3'][0][..., q]), 4 * UDD, qr)
        # the factor is the same in both passes
        assert np.array_equal(g3['raw']['D'], g['raw']['D']) and np.array_equal(g3['raw']['Dl'], g['raw']['Dl'])


def test_dd_low_words_of_the_input(h):
    """a matrix given as hi + lo: the low words of D and Ccpl enter the factorisation (a kernel that read the high words only would solve another system: residual ~1e-17)"""
    p, d, cond = 3, 78, 1e8
    c = cr.case(p, d, cond)
    rng = np.random.default_rng(5)
    D, Cc = c['D'][0], c['Cc'][0]
    S = rng.standard_normal((p, d, d)); S = S + S.transpose(0, 2, 1)
    Dlo = D * 2.0 ** -55 * S; Clo = Cc * 2.0 ** -54 * rng.standard_normal((p, d, d))
    g = h.debug_block_factor(c['D'], c['Cc'], c['b1'], dd=True, Dlo=Dlo[None], Clo=Clo[None])
    assert g['nshift'][0] == 0
    r = cr.reference_dd(_sched(p), D, Cc, c['b1'][0], Dlo, Clo)
    qr = _dd_quotient(D, Cc, r['xh'], r['xl'], c['b1'][0], Dlo, Clo)
    check('f dd residual with low input words', _dd_quotient(D, Cc, g['x'][0], g['xl'][0], c['b1'][0], Dlo, Clo), 4 * UDD, qr)
    assert _dd_quotient(D, Cc, g['x'][0], g['xl'][0], c['b1'][0]) > 1e6 * 4 * UDD                       # (measured against hi alone it is another system)


def test_dd_forward_error_against_mpmath(h):
    """one small system (50 unknowns) at cond(T) ~ 1e12: an fp64-accurate answer is off by ~cond * 1e-16 = 1e-4 there, a double-double one by cond * 1e-32"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 70
    p, d, cond = 5, 10, 1e12
    c = cr.case(p, d, cond)
    D, Cc, b = c['D'][0], c['Cc'][0], c['b1'][0]
    g = h.debug_block_factor(c['D'], c['Cc'], c['b1'], dd=True)
    T = cr.dense(D, Cc)                                      # (p = 5: no two blocks coincide, the fp64 assembly is exact)
    xm = mp.lu_solve(mp.matrix(T.tolist()), mp.matrix(b.ravel().tolist()))
    xg = [mp.mpf(float(a)) + mp.mpf(float(l)) for a, l in zip(g['x'][0].ravel(), g['xl'][0].ravel())]
    fe = float(mp.sqrt(sum((xg[i] - xm[i]) ** 2 for i in range(p * d))) / mp.sqrt(sum(xm[i] ** 2 for i in range(p * d))))
    check(f'f dd forward error p{p} d{d} cond {c["cond"][0]:.1e}', fe, c['cond'][0] * 4 * UDD)


def test_dd_listed_sub_batch(h):
    """four distinct systems, the list [2, 0]: the unlisted problems keep every word that was uploaded, the listed ones equal the same problem alone"""
    p, d, cond = 3, 78, 1e8
    c = cr.case(p, d, cond, nb=4)
    keys = ('D', 'O', 'F', 'Ddiag', 'X', 'Dl', 'Ol', 'Fl', 'Xl')
    out = h.debug_block_factor(c['D'], c['Cc'], c['b1'], plist=[2, 0], dd=True)
    up = h.debug_block_factor(c['D'], c['Cc'], c['b1'], plist=[], dd=True)
    assert not out['nshift'].any()
    for b in (1, 3):
        for k in keys:
            assert np.array_equal(out['raw'][k][b], up['raw'][k][b]), (b, k)
    for b in (2, 0):
        alone = h.debug_block_factor(c['D'][b:b + 1], c['Cc'][b:b + 1], c['b1'][b:b + 1], dd=True)
        for k in keys:
            assert np.array_equal(out['raw'][k][b], alone['raw'][k][0]), (b, k)
        r = cr.reference_dd(_sched(p), c['D'][b], c['Cc'][b], c['b1'][b])
        qr = _dd_quotient(c['D'][b], c['Cc'][b], r['xh'], r['xl'], c['b1'][b])
        check(f'f dd residual listed problem{b}', _dd_quotient(c['D'][b], c['Cc'][b], out['x'][b], out['xl'][b], c['b1'][b]), 4 * UDD, qr)
