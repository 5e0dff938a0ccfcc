"""Float32 triangular solves with both edges of a node in one workgroup (round 9; TMPC_TUNE_TRSM_PAIR, tmpc_cr.h: trf_strip<2>; run with -m gpu).

With the key on, an item of k_cr_trsm_dma_f32 is (problem, eliminated node, 64-row strip): the strip of BOTH edge blocks of the node is solved on one stream
of the node's factor, every L fragment read and rounded once.  Every output element sees the MFMA sequence of the one-edge form in the same k order, so the
claim under test is bit identity, not a tolerance: every image a factorisation leaves (D, O, F, Ddiag, X, O32) is np.array_equal with the key on and off --
for every case of cr_reference.F32_CASES (block widths with one full tile and a 16-wide one, 48-wide last tiles and strips, five full tiles; p = 2 without
a two-edge node, p >= 3 with two-edge nodes, the one-edge node and the fill accumulation), in mixed float32 / fp64 batches under a permuted list, and
through a whole interior-point solve.  tmpc_debug_last_trsm_pairs (a host-side count of the two-edge items the call launched) shows that the path ran:
a test that passes with the switch ignored proves nothing."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch ships its own HIP runtime and fails to find the GPU when it initialises second)

pytestmark = pytest.mark.gpu

import cr_reference as cr  # noqa: E402

RAW_KEYS = ('D', 'O', 'F', 'Ddiag', 'X', 'O32')
KINDS = ('pass2', 'fused')


@pytest.fixture(scope='module')
def h():
    from tunempc_amd._lib import HipConvexifier
    hh = HipConvexifier(2, 3, 1)
    yield hh
    hh.close()


def _sched(p):
    from tunempc_amd._lib import cr_schedule
    return cr_schedule(p)


def _expected_pairs(p, d, nlowp):
    """two-edge items of one factorisation: (nodes with both edges, on the levels that have updates) x 64-row strips x float32 problems of the list"""
    sched = _sched(p)
    nst = ((d + 15) // 16 * 16 + 63) // 64
    n2 = 0
    for eoff, nelim, _uoff, nupd in sched['levels']:
        if nupd:
            n2 += sum(1 for rec in sched['elim'][eoff:eoff + nelim] if int(rec[3]) >= 0 and int(rec[4]) >= 0)
    return n2 * nst * nlowp


def _factor(h, pair, *args, **kw):
    """(result, two-edge items launched) of one debug_block_factor with the key set to `pair`; the handle goes back to the default"""
    h.set_tuning(trsm_pair=pair)
    try:
        out = h.debug_block_factor(*args, **kw)
        return out, h.debug_last_trsm_pairs()
    finally:
        h.set_tuning(trsm_pair=1)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('p,d,cond', cr.F32_CASES)
def test_pair_on_equals_pair_off(h, p, d, cond, kind):
    c = cr.case(p, d, cond)
    rhs = c['b1'] if kind == 'pass2' else c['b3']
    kw = dict(lowp=[1], lowp_trsm=True, pass1=kind != 'pass2', fuse_fwd1=kind == 'fused')
    on, n_on = _factor(h, 1, c['D'], c['Cc'], rhs, **kw)
    off, n_off = _factor(h, 0, c['D'], c['Cc'], rhs, **kw)
    # the path ran (and only where a node has two edges), the switch is honoured
    want = _expected_pairs(p, d, 1)
    print(f'FIG pairs p{p} d{d} {kind}: on {n_on} off {n_off} expected {want}')
    assert n_off == 0 and n_on == want
    assert (n_on > 0) == (p >= 3)
    assert on['nshift'][0] == 0 and off['nshift'][0] == 0
    for k in RAW_KEYS:
        assert np.array_equal(on['raw'][k], off['raw'][k]), k
    # the solve ran in float32 (O32 is not the zero it was created as), and its padding is exactly zero: rows and columns d .. dp / ld32
    o32 = on['raw']['O32']
    assert np.any(o32[:, :, :d, :d] != 0.0)
    assert not o32[:, :, d:, :].any() and not o32[:, :, :, d:].any()


def test_key_off_and_fp64_launch_no_pairs(h):
    """the count is of THIS call: zero with the key off, zero without float32 solves, zero for a float32 problem that is not on the list"""
    p, d, cond = cr.F32_CASES[1]
    c = cr.case(p, d, cond)
    assert _factor(h, 1, c['D'], c['Cc'], c['b1'], lowp=[1], lowp_trsm=True)[1] == _expected_pairs(p, d, 1) > 0
    assert _factor(h, 0, c['D'], c['Cc'], c['b1'], lowp=[1], lowp_trsm=True)[1] == 0
    assert _factor(h, 1, c['D'], c['Cc'], c['b1'], lowp=[1], lowp_trsm=False)[1] == 0          # float32 updates, fp64 solves
    assert _factor(h, 1, c['D'], c['Cc'], c['b1'])[1] == 0                                       # fp64 throughout
    assert _factor(h, 1, c['D'], c['Cc'], c['b1'], plist=[], lowp=[1], lowp_trsm=True)[1] == 0   # nothing listed: no kernel


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('p,d,cond', cr.LIST_CASES)
def test_mixed_batch(h, p, d, cond, kind):
    """six systems, float32 members 0, 2, 3, 5 and fp64 members 1, 4 under a permuted list: key on equals key off bit for bit; each float32 member equals the same
    system run alone; the fp64 members equal a call without any float32 member"""
    c = cr.case(p, d, cond, nb=6)
    rhs = c['b1'] if kind == 'pass2' else c['b3']
    kw = dict(pass1=kind != 'pass2', fuse_fwd1=kind == 'fused')
    lowp = np.array([1, 0, 1, 1, 0, 1], np.int32)
    plist = [3, 0, 5, 4, 2, 1]
    on, n_on = _factor(h, 1, c['D'], c['Cc'], rhs, plist=plist, lowp=lowp, lowp_trsm=True, **kw)
    off, n_off = _factor(h, 0, c['D'], c['Cc'], rhs, plist=plist, lowp=lowp, lowp_trsm=True, **kw)
    assert n_off == 0 and n_on == _expected_pairs(p, d, 4) > 0
    assert not on['nshift'].any()
    for k in RAW_KEYS:
        assert np.array_equal(on['raw'][k], off['raw'][k]), k
    for b in (0, 2, 3, 5):
        alone, n1 = _factor(h, 1, c['D'][b:b + 1], c['Cc'][b:b + 1], rhs[b:b + 1], lowp=[1], lowp_trsm=True, **kw)
        assert n1 == _expected_pairs(p, d, 1)
        for k in RAW_KEYS:
            assert np.array_equal(on['raw'][k][b], alone['raw'][k][0]), (b, k)
    allf, n64 = _factor(h, 1, c['D'], c['Cc'], rhs, plist=plist, **kw)
    assert n64 == 0
    for b in (1, 4):
        for k in RAW_KEYS[:-1]:
            assert np.array_equal(on['raw'][k][b], allf['raw'][k][b]), (b, k)
        assert not on['raw']['O32'][b].any()
    assert not np.array_equal(on['raw']['X'][0], allf['raw']['X'][0])       # (the float32 members are not the fp64 ones: their kernels ran)


def test_whole_solve_is_bit_identical():
    """the bench stage shape (nx = 24, mb = 8: blocks of 300) at a period of six, four problems in one chunk: every output of the solve with the key on and off"""
    from tunempc_amd import synthetic
    from tunempc_amd._lib import HipConvexifier
    A, B, H = synthetic.gen_batch(90, 4, 6, 24, 8)
    outs = []
    for tune in (dict(trsm_pair=1), dict(trsm_pair=0), dict(lowp_trsm=0)):
        hc = HipConvexifier(6, 24, 8, chunk=4)
        try:
            hc.set_tuning(**tune)
            outs.append(hc.convexify_batch(A, B, H))
        finally:
            hc.close()
    on, off, fp64_solves = outs
    assert np.all(on['status'] == 0)
    for k in ('Hc', 'dHc', 'P', 'kappa', 'iters', 'status'):
        assert np.array_equal(on[k], off[k]), k
    # float32 solves did run in these solves (else the key had nothing to switch): without them the point moves in its last bits
    assert not np.array_equal(on['Hc'], fp64_solves['Hc'])
