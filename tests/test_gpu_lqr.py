"""GPU tests of the periodic LQR kernel (csrc/tmpc_lqr.h) and of the feedback-equivalence certificate (tunempc_amd/lqr.py) against the numpy statement of
the recursion in tests/lqr_reference.py.  The entries are handle-free; relative errors are relative Frobenius norms per problem (the project's parity
measure), the bar is the project's parity bar 1e-8."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded: torch ships its own HIP runtime and fails to find the GPU when it initialises second)

pytestmark = pytest.mark.gpu

import lqr_reference as lr  # noqa: E402
from tunempc_amd.synthetic import gen_batch  # noqa: E402

PARITY = 1e-8
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def sweeps_close(a, b):
    return abs(int(a) - int(b)) <= 2 + 0.05 * max(int(a), int(b))


def check_parity(tag, A, B, H, Pi0=None):
    """The kernel against numpy on one batch: status 0, K, Pi, Phi to 1e-8 relative, sweeps within 2 + 5 %.  Returns the kernel's dict."""
    from tunempc_amd import lqr
    out = lqr.periodic_lqr_batch(A, B, H, Pi0=Pi0)
    ref = lr.periodic_lqr_batch(A, B, H, Pi0=Pi0)
    worst = dict(K=0.0, Pi=0.0, Phi=0.0)
    for b, r in enumerate(ref):
        assert r['converged'], (tag, b)
        e = {k: rel(out[k][b], r[k]) for k in worst}
        worst = {k: max(worst[k], e[k]) for k in worst}
        assert int(out['status'][b]) == 0, (tag, b, out['info'][b])
        assert e['K'] <= PARITY and e['Pi'] <= PARITY and e['Phi'] <= PARITY, (tag, b, e)
        assert sweeps_close(out['sweeps'][b], r['sweeps']), (tag, b, out['sweeps'][b], r['sweeps'])
        assert abs(out['rho'][b] - r['rho']) <= PARITY * max(1.0, r['rho']), (tag, b, out['rho'][b], r['rho'])
    print('%-34s nb %3d  sweeps gpu %s numpy %s  rel err K %.1e Pi %.1e Phi %.1e  min eig S %.2f  posdef last / path %s' % (
        tag, len(ref), sorted(set(out['sweeps'].tolist())), sorted({r['sweeps'] for r in ref}), worst['K'], worst['Pi'], worst['Phi'],
        min(r['smin'] for r in ref), sorted(set(map(tuple, out['info'][:, 5:7].tolist())))))
    return out


# ----------------------------------------------------------------------------- 1. parity with the numpy reference
@pytest.mark.parametrize('name', lr.GOLDENS)
@pytest.mark.parametrize('side', ['H', 'Hc'])
def test_parity_on_goldens(name, side):
    """Every golden of the plain model, the indefinite H and the convexified Hc (from zero S turns indefinite on the H side of the AWE, identity-family and
    c5 vectors: a Cholesky-only solve would fail them)."""
    g = lr.load_golden(name)
    check_parity(name + ':' + side, g['A'], g['B'], g[side])


@pytest.mark.parametrize('seed,nb,p,nx,mb', [(7, 16, 64, 24, 8), (11, 256, 50, 2, 2), (11, 8, 1, 4, 2), (11, 1, 3, 31, 1), (11, 1, 2, 1, 31)])
def test_parity_on_generated_batches(seed, nb, p, nx, mb):
    """The bench stage shape, a wide batch of small problems, p = 1, and the two extreme splits of n = 32."""
    A, B, H = gen_batch(seed, nb, p, nx, mb)
    check_parity('gen_batch(%d,%d,%d,%d,%d)' % (seed, nb, p, nx, mb), A, B, H)


@pytest.mark.parametrize('seed,nb,p,nx,mb', [(11, 2, 3, 40, 20), (11, 1, 2, 63, 1), (11, 1, 2, 1, 63), (11, 1, 2, 32, 32)])
def test_parity_on_blocks_beyond_32(seed, nb, p, nx, mb):
    """32 < nx + nu <= 64 runs on the same kernel (all operands still fit the LDS: 131 KB at nx = 63)."""
    A, B, H = gen_batch(seed, nb, p, nx, mb)
    check_parity('gen_batch(%d,%d,%d,%d,%d)' % (seed, nb, p, nx, mb), A, B, H)


# ----------------------------------------------------------------------------- 2. Pi0
@pytest.mark.parametrize('name', lr.GOLDENS)
def test_start_from_P_follows_the_convexified_path(name):
    """Hc_k = H_k + calH_k(P), so the H side started from Pi0 = +P runs the iterates of the Hc side shifted by P.  Checked three ways:
    (a) after the same three sweeps (tol = 0, max_sweeps = 3) Pi(H) - P = Pi(Hc), same gains, same pivots of S;
    (b) run to convergence, the sweep count of the Hc side is reproduced exactly;
    (c) info[6] (S positive definite on the whole path) reads 1 from P where the zero start of the AWE and c5 vectors reads 0.
    (b) has one exception, stated here with its figures: the stop measure max|dPi_k| / max(1, max|Pi_k|) is not shift invariant.  On c1 max|Pi| is 1.29 on the
    H side and 0.87 on the Hc side, the change per sweep shrinks by only 12 %, and the H side stops at sweep 211 where the Hc side needs 214 (numpy: the same two
    figures).  Everywhere else convergence is far too fast for the denominators to matter.  c1 is held to the sweep bar of the parity tests, 2 + 5 %."""
    from tunempc_amd import lqr
    g = lr.load_golden(name)
    fP = lqr.periodic_lqr_batch(g['A'], g['B'], g['H'], Pi0=g['P'], tol=0.0, max_sweeps=3)
    fC = lqr.periodic_lqr_batch(g['A'], g['B'], g['Hc'], tol=0.0, max_sweeps=3)
    for b in range(g['A'].shape[0]):
        assert rel(fP['Pi'][b] - g['P'][b], fC['Pi'][b]) <= PARITY and rel(fP['K'][b], fC['K'][b]) <= PARITY
        assert rel(fP['info'][b, 3:5], fC['info'][b, 3:5]) <= PARITY
    oP = check_parity(name + ':H from P', g['A'], g['B'], g['H'], Pi0=g['P'])
    oC = lqr.periodic_lqr_batch(g['A'], g['B'], g['Hc'])
    o0 = lqr.periodic_lqr_batch(g['A'], g['B'], g['H'])
    print(name, 'sweeps from P', oP['sweeps'], 'Hc side', oC['sweeps'], 'posdef on the path from P', oP['info'][:, 6], 'from 0', o0['info'][:, 6], 'Hc', oC['info'][:, 6])
    if name == 'c1_convex_lqr':
        assert sweeps_close(oP['sweeps'][0], oC['sweeps'][0])
    else:
        assert (oP['sweeps'] == oC['sweeps']).all()
    assert (oP['info'][:, 5:7] == 1.0).all() and (oC['info'][:, 5:7] == 1.0).all()
    assert (o0['info'][:, 5] == 1.0).all()           # at the converged Pi the S of the H side IS the S of the Hc side
    if name in ('awe_shape_n15', 'c5_awe_synthetic_p200_n30'):
        assert (o0['info'][:, 6] == 0.0).all()
    for b in range(g['A'].shape[0]):
        assert rel(oP['Pi'][b], oC['Pi'][b] + g['P'][b]) <= PARITY and rel(oP['K'][b], oC['K'][b]) <= PARITY


# ----------------------------------------------------------------------------- 3. host entry == device entry
@pytest.mark.parametrize('with_pi0', [False, True])
def test_host_and_device_entries_return_the_same_bits(with_pi0):
    from tunempc_amd import lqr
    g = lr.load_golden('mid_n16')
    A, B, H = gen_batch(7, 3, 64, 24, 8)
    for a, b_, h, p0 in ((g['A'], g['B'], g['H'], g['P']), (A, B, H, 0.1 * np.tile(np.eye(24), (3, 64, 1, 1)))):
        p0 = p0 if with_pi0 else None
        host = lqr.periodic_lqr_batch(a, b_, h, Pi0=p0)
        t = lambda x: None if x is None else torch.from_numpy(x).cuda()
        dev = lqr.periodic_lqr_batch(t(a), t(b_), t(h), Pi0=t(p0))
        for k in ('K', 'Pi', 'Phi', 'info', 'status', 'sweeps'):
            assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
            np.testing.assert_array_equal(dev[k].cpu().numpy(), host[k], err_msg=k)
        np.testing.assert_array_equal(dev['rho'], host['rho'])


# ----------------------------------------------------------------------------- 4. statuses
def test_max_sweeps_gives_status_1_and_a_finite_partial_iterate():
    from tunempc_amd import lqr
    g = lr.load_golden('c1_convex_lqr')
    out = lqr.periodic_lqr_batch(g['A'], g['B'], g['H'], max_sweeps=5)
    ref = lr.periodic_lqr(g['A'][0], g['B'][0], g['H'][0], max_sweeps=5)
    assert int(out['status'][0]) == 1 and int(out['sweeps'][0]) == 5 and out['info'][0, 2] > 1e-13
    for k in ('K', 'Pi', 'Phi'):
        assert np.isfinite(out[k]).all() and rel(out[k][0], ref[k]) <= PARITY
    assert np.isfinite(out['rho'][0])


def test_diverging_member_stops_with_a_status_and_leaves_the_batch_alone():
    """B = 0 with an expanding A: Pi grows by 4 per sweep and overflows near sweep 512 -> status 3 at that sweep (not max_sweeps later); the other members of the
    batch return what they return alone, bit for bit."""
    from tunempc_amd import lqr
    A, B, H = gen_batch(11, 3, 1, 2, 1)
    A[1, 0] = np.diag([2.0, 0.5]); B[1] = 0.0; H[1, 0] = np.eye(3)
    out = lqr.periodic_lqr_batch(A, B, H)
    print('statuses', out['status'], 'sweeps', out['sweeps'], 'info[1]', out['info'][1])
    assert int(out['status'][1]) in (1, 3)
    if int(out['status'][1]) == 3:
        assert int(out['sweeps'][1]) < 600 and np.isnan(out['rho'][1])
    keep = [0, 2]
    solo = lqr.periodic_lqr_batch(A[keep], B[keep], H[keep])
    assert (out['status'][keep] == 0).all()
    for k in ('K', 'Pi', 'Phi', 'info'):
        np.testing.assert_array_equal(out[k][keep], solo[k], err_msg=k)
    check_parity('members beside a diverging one', A[keep], B[keep], H[keep])


def test_singular_S_gives_status_2():
    """H = 0 and B = 0 at stage 0: S = R_0 + B_0' Pi_1 B_0 = 0 -> status 2 for that member, the other one converges."""
    from tunempc_amd import lqr
    A, B, H = gen_batch(11, 2, 2, 2, 1)
    B[0, 0] = 0.0; H[0, 0] = 0.0
    out = lqr.periodic_lqr_batch(A, B, H)
    print('statuses', out['status'], 'info[0]', out['info'][0])
    assert int(out['status'][0]) == 2 and int(out['sweeps'][0]) == 1 and np.isnan(out['rho'][0])
    assert int(out['status'][1]) == 0
    solo = lqr.periodic_lqr_batch(A[1:], B[1:], H[1:])
    np.testing.assert_array_equal(out['K'][1], solo['K'][0])


# ----------------------------------------------------------------------------- 5. end to end: the convexified scheme has the feedback law of the indefinite one
def _certify(tag, A, B, H, res):
    from tunempc_amd import lqr
    opt = np.asarray(res['status']) == 0
    assert opt.any(), tag
    worst = 0.0
    for P in (None, res['P']):
        c = lqr.feedback_equivalence_batch(A, B, H, res['Hc'], P=P)
        print('%-28s P %-5s dK %.2e dK_rel %.2e  rho_H max %.3g rho_Hc max %.3g  sweeps H %s Hc %s  posdef_H %s  Optimal %d / %d' % (
            tag, P is not None, c['dK'][opt].max(), c['dK_rel'][opt].max(), np.max(c['rho_H'][opt]), np.max(c['rho_Hc'][opt]),
            sorted(set(c['sweeps_H'].tolist())), sorted(set(c['sweeps_Hc'].tolist())), sorted(set(c['posdef_H'].tolist())), opt.sum(), opt.size))
        assert (c['status_H'][opt] == 0).all() and (c['status_Hc'][opt] == 0).all()
        assert (c['dK'][opt] <= PARITY).all()
        assert (c['rho_H'][opt] < 1.0).all() and (c['rho_Hc'][opt] < 1.0).all()
        worst = max(worst, c['dK'][opt].max())
    return worst


def test_certificate_after_convexify_batch_at_the_bench_stage_shape():
    from tunempc_amd import convexifier
    A, B, H = gen_batch(7, 16, 64, 24, 8)
    res = convexifier.convexify_batch(A, B, H)
    assert (res['status'] == 0).all()
    _certify('bench shape 16 x (64,24,8)', A, B, H, res)


@pytest.mark.parametrize('name', ['c2_unicycle_shape', 'c3_evaporation_shape'])
def test_certificate_after_convexify_batch_at_small_shapes(name):
    from tunempc_amd import convexifier
    g = lr.load_golden(name)
    res = convexifier.convexify_batch(g['A'], g['B'], g['H'])
    assert (res['status'] == 0).all()
    _certify(name, g['A'], g['B'], g['H'], res)


def test_certificate_after_device_resident_convexify():
    """torch tensors all the way: convexify_batch_device, then the certificate on its outputs without a host copy of A / B / H."""
    from tunempc_amd import lqr
    from tunempc_amd._lib import HipConvexifier
    A, B, H = (torch.from_numpy(x).cuda() for x in gen_batch(7, 4, 64, 24, 8))
    h = HipConvexifier(64, 24, 8, chunk=4)
    res = h.convexify_batch_device(A, B, H)
    torch.cuda.synchronize()
    assert (res['status'] == 0).all()
    c = lqr.feedback_equivalence_batch(A, B, H, res['Hc'], P=res['P'])
    assert isinstance(c['K'], torch.Tensor) and c['K'].is_cuda
    assert (c['dK'] <= PARITY).all() and (c['rho_H'] < 1.0).all() and (c['rho_Hc'] < 1.0).all() and (c['posdef_H'] == 1.0).all()
    h.close()


def test_certificate_through_the_dropin_convexify_on_c1():
    """examples/convex_lqr.py:52-58 with the library's own gains: convexify, then K(H) against K(H + dHc) -- 1e-8 where the reference asks 1e-5 --, and the gain
    agrees with scipy's DARE gain."""
    import scipy.linalg as sla
    from tunempc_amd import convexifier, lqr
    g = np.load(os.path.join(GOLDEN, 'c1_convex_lqr.npz'))
    A = np.matrix(g['A'][0, 0]); B = np.matrix(g['B'][0, 0]); Q = np.matrix(g['Q']); R = np.matrix(g['R']); N = np.matrix(g['N'])
    dHc, dQc, dRc, dNc = convexifier.convexify(A, B, Q, R, N)
    c = lqr.feedback_equivalence(A, B, Q, R, N, dHc)
    print('c1 drop-in: dK %.2e rho %.4f %.4f sweeps %d %d' % (c['dK'], c['rho_H'], c['rho_Hc'], c['sweeps_H'], c['sweeps_Hc']))
    assert c['status_H'] == 0 and c['status_Hc'] == 0 and c['dK'] <= PARITY and c['rho_H'] < 1.0 and c['rho_Hc'] < 1.0
    K, Pi, rho = lqr.periodic_lqr(A, B, Q, R, N)
    An, Bn, Qn, Rn, Nn = (np.asarray(x) for x in (A, B, Q, R, N))
    X = sla.solve_discrete_are(An, Bn, Qn, Rn, s=Nn)
    Kref = np.linalg.solve(Rn + Bn.T @ X @ Bn, Bn.T @ X @ An + Nn.T)
    assert len(K) == 1 and np.abs(K[0] - Kref).max() <= 1e-9 and np.abs(Pi[0] - X).max() <= 1e-9 * np.abs(X).max() and rho < 1.0
    assert np.abs(c['K'][0] - Kref).max() <= 1e-9


# ----------------------------------------------------------------------------- 6. Step 3 (force): the certificate measures what T_k changed
def test_step3_golden_call_agrees_with_numpy():
    """tests/golden/n1_step3_force.npz (N = 0, both gains ~ 0: a weak case): the list-style call works and agrees with numpy."""
    from tunempc_amd import lqr
    g = np.load(os.path.join(GOLDEN, 'n1_step3_force.npz'))
    p = g['A'].shape[0]
    lists = [[g[k][i] for i in range(p)] for k in ('A', 'B', 'Q', 'R', 'N')]
    c = lqr.feedback_equivalence(*lists, [g['dHc'][i] for i in range(p)])
    nx = g['A'].shape[1]
    H = np.zeros_like(g['dHc'])
    H[:, :nx, :nx] = g['Q']; H[:, nx:, nx:] = g['R']; H[:, :nx, nx:] = g['N']; H[:, nx:, :nx] = np.swapaxes(g['N'], 1, 2)
    rH = lr.periodic_lqr(g['A'], g['B'], H); rC = lr.periodic_lqr(g['A'], g['B'], H + g['dHc'])
    print('n1_step3_force: dK', c['dK'], 'numpy', np.abs(rH['K'] - rC['K']).max(), 'sweeps', c['sweeps_H'], c['sweeps_Hc'], rH['sweeps'], rC['sweeps'])
    assert c['status_H'] == 0 and c['status_Hc'] == 0 and rH['converged'] and rC['converged']
    assert np.abs(np.stack(c['K']) - rH['K']).max() <= PARITY and np.abs(np.stack(c['Kc']) - rC['K']).max() <= PARITY
    assert abs(c['dK'] - np.abs(rH['K'] - rC['K']).max()) <= PARITY


def test_step3_generated_certificate_equals_numpy():
    """convexify_step3_batch on 4 generated problems: dHc contains T_k, so dK is a measurement, not a bound -- finite and equal to numpy's."""
    from tunempc_amd import convexifier, lqr
    A, B, H = gen_batch(11, 4, 6, 6, 2)
    res = convexifier.convexify_step3_batch(A, B, H, 1e-3)
    c = lqr.feedback_equivalence_batch(A, B, H, res['Hc'])
    for b in range(4):
        rH = lr.periodic_lqr(A[b], B[b], H[b]); rC = lr.periodic_lqr(A[b], B[b], res['Hc'][b])
        dref = np.abs(rH['K'] - rC['K']).max()
        print('step 3 member', b, 'status', int(res['status'][b]), 'dK', c['dK'][b], 'numpy', dref, 'max T', np.abs(res['T'][b]).max())
        assert rH['converged'] and rC['converged'] and int(c['status_H'][b]) == 0 and int(c['status_Hc'][b]) == 0
        assert np.isfinite(c['dK'][b])
        assert abs(c['dK'][b] - dref) <= PARITY * max(dref, np.abs(rC['K']).max())
        assert rel(c['K'][b], rH['K']) <= PARITY and rel(c['Kc'][b], rC['K']) <= PARITY


# ----------------------------------------------------------------------------- 7. refusals
def test_blocks_beyond_64_are_refused_with_the_library_message():
    from tunempc_amd import lqr
    A = np.zeros((1, 2, 50, 50)); B = np.zeros((1, 2, 50, 15)); H = np.tile(np.eye(65), (1, 2, 1, 1))
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64 \\(got 65\\)'):
        lqr.periodic_lqr_batch(A, B, H)
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64 \\(got 65\\)'):
        lqr.periodic_lqr_batch(*(torch.from_numpy(x).cuda() for x in (A, B, H)))
    with pytest.raises(ValueError, match='one GPU'):
        lqr.periodic_lqr_batch(*(torch.from_numpy(x) for x in (A, B, H)))
