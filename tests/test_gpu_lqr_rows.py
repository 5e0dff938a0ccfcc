"""GPU tests of the periodic LQ recursion with rows (csrc/tmpc_lqr_rows.h, the J= / ncnt= / ng= arguments of tunempc_amd/lqr.py) and of the feedback-
equivalence certificate for the models with rows, against the numpy statement in tests/lqr_rows_reference.py (its null-space form: not the kernel's method).
Relative errors are relative Frobenius norms per problem; the bar is the project's parity bar 1e-8 (tests/test_gpu_lqr.py).

Figures measured on the CPU before these tests were written (numpy on oracle/cpu_ipm solutions): the constrained dK is 3e-15 ... 2e-12 where the
unconstrained one is 0.11 ... 0.24 at multipliers 0.13 ... 1.9.

Choice of the small Step 2 batch (p 8, nx 6, nu 4, 1 + 0..2 rows): synthetic.gen_batch(21, 3, ...) with rows of seed 22, not the seeds 5 / 6 of the CPU tests.
Member 0 of that batch has max|Pi| = 3.7e4 at a KKT condition of 1e6: the change of Pi per sweep stalls at 1e-13 relative -- rounding noise -- and the sweep at
which the tol = 1e-13 stop is met is a lottery (numpy: 19 / 13 sweeps in the null-space form, 227 / 65 in the KKT form, 7 in both at tol = 1e-12), so the
sweep-count rule of the parity tests says nothing there.  check_parity therefore asserts, as part of the qualification of a batch, that the two forms of the
numpy reference themselves stop within that rule; seeds 21 / 22 (multipliers 0.8 ... 1.9, 6 sweeps, max|Pi| < 100) do, as does every other batch below."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_rows_reference as lrr  # noqa: E402
from tunempc_amd.synthetic import gen_batch  # noqa: E402

PARITY = 1e-8
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def sweeps_close(a, b):
    return abs(int(a) - int(b)) <= 2 + 0.05 * max(int(a), int(b))


@pytest.fixture
def hc():
    """Handles of ONE test, each sized for the batch it solves and closed when the test ends, pass or fail."""
    from tunempc_amd._lib import HipConvexifier
    made = []

    def get(p, nx, mb, chunk, **kw):
        made.append(HipConvexifier(p, nx, mb, chunk=chunk, **kw))
        return made[-1]
    yield get
    for h in made:
        h.close()


def optimal_members(tag, status, cap=16):
    """The members a solve ended Optimal on; the others are excluded by count, at most 1 in `cap`."""
    opt = np.asarray(status) == 0
    excluded = int((~opt).sum())
    print('%s: %d of %d members not Optimal (excluded)' % (tag, excluded, opt.size))
    assert excluded * cap <= opt.size, (tag, np.asarray(status))
    return np.flatnonzero(opt)


def step2_solution(hc, seed, rseed, nb, p, nx, mb, ng, nc, rho):
    A, B, H = gen_batch(seed, nb, p, nx, mb)
    J, ncnt = lrr.gen_rows(rseed, nb, p, nx + mb, ng, nc)
    o = hc(p, nx, mb, nb, ng=ng, nc=nc).convexify_step2_batch(A, B, H, J, ncnt, rho)
    return A, B, H, J, ncnt, o


def check_parity(tag, A, B, H, J, ncnt, ng, Pi0=None, **kw):
    """The kernel against numpy on one batch: status 0, K, Pi, Phi, Lam to 1e-8 relative, sweeps within 2 + 5 %, the gains feasible.  The batch qualifies as
    a parity case only if numpy converges in well under max_sweeps with max|Pi| < 1e5 and its two forms stop at the same sweep within the rule (asserted: the
    data are chosen, not filtered)."""
    from tunempc_amd import lqr
    out = lqr.periodic_lqr_batch(A, B, H, Pi0=Pi0, J=J, ncnt=ncnt, ng=ng, **kw)
    rows = ng + (ncnt if ncnt is not None else np.zeros(A.shape[:2], int))
    ref = lrr.periodic_lqr_batch(A, B, H, J, rows, Pi0=Pi0, **kw)
    kkt = lrr.periodic_lqr_batch(A, B, H, J, rows, Pi0=Pi0, method='kkt', **kw)
    worst = dict(K=0.0, Pi=0.0, Phi=0.0, Lam=0.0)
    for b, r in enumerate(ref):
        assert r['converged'] and r['sweeps'] <= 500 and np.abs(r['Pi']).max() < 1e5, (tag, b, r['sweeps'], np.abs(r['Pi']).max())
        assert kkt[b]['converged'] and sweeps_close(kkt[b]['sweeps'], r['sweeps']), (tag, b, kkt[b]['sweeps'], r['sweeps'])      # the stop is not decided by rounding
        e = {k: rel(out[k][b], r[k]) for k in worst}
        worst = {k: max(worst[k], e[k]) for k in worst}
        print('   member %d: sweeps gpu %d numpy %d  rel err %s  feas %.1e  info %s' % (b, out['sweeps'][b], r['sweeps'], e, out['feas'][b], out['info'][b].tolist()))
        assert int(out['status'][b]) == 0, (tag, b, out['info'][b])
        assert e['K'] <= PARITY and e['Pi'] <= PARITY and e['Phi'] <= PARITY and e['Lam'] <= PARITY, (tag, b, e)
        assert sweeps_close(out['sweeps'][b], r['sweeps']), (tag, b, out['sweeps'][b], r['sweeps'])
        assert abs(out['rho'][b] - r['rho']) <= PARITY * max(1.0, r['rho']), (tag, b, out['rho'][b], r['rho'])
        assert out['feas'][b] <= 1e-9 * max(1.0, np.abs(out['K'][b]).max()), (tag, b, out['feas'][b])
        for k in range(A.shape[1]):
            assert not out['Lam'][b, k, rows[b, k]:].any()
    print('%-40s nb %3d  rows %d..%d  sweeps gpu %s numpy %s  rel err K %.1e Pi %.1e Phi %.1e Lam %.1e  convex last / path %s' % (
        tag, len(ref), rows.min(), rows.max(), sorted(set(out['sweeps'].tolist())), sorted({r['sweeps'] for r in ref}), worst['K'], worst['Pi'], worst['Phi'],
        worst['Lam'], sorted(set(map(tuple, out['info'][:, 5:7].tolist())))))
    return out


# ----------------------------------------------------------------------------- 4. parity with the numpy reference
@pytest.mark.parametrize('seed,rseed,nb,p,nx,mb,ng,nc', [(21, 22, 3, 8, 6, 4, 1, 2), (61000, 61, 2, 64, 24, 8, 2, 3)])
def test_parity_on_step2_solutions_both_sides(hc, seed, rseed, nb, p, nx, mb, ng, nc):
    """Rows, Hc and P of a Step 2 solve with active multipliers (rho = 1e-3): the H side from Pi0 = P and the Hc side from zero, ragged ncnt."""
    A, B, H, J, ncnt, o = step2_solution(hc, seed, rseed, nb, p, nx, mb, ng, nc, 1e-3)
    m = optimal_members('step 2 (%d,%d,%d)' % (p, nx, mb), o['status'])
    A, B, H, J, ncnt, Hc, P = (x[m] for x in (A, B, H, J, ncnt, o['Hc'], o['P']))
    tag = '(%d,%d,%d; %d + 0..%d)' % (p, nx, mb, ng, nc)
    oH = check_parity(tag + ' H from P', A, B, H, J, ncnt, ng, Pi0=P)
    oC = check_parity(tag + ' Hc from zero', A, B, Hc, J, ncnt, ng)
    assert (oC['info'][:, 5:7] == 1.0).all()                # every stage problem of the Hc side shown convex
    for b in range(len(m)):
        assert rel(oH['K'][b], oC['K'][b]) <= PARITY and rel(oH['Pi'][b], oC['Pi'][b] + P[b]) <= PARITY


def test_parity_with_stages_without_rows_and_with_as_many_rows_as_inputs():
    """Random rows on the Hc / P of a plain solve, (8, 6, 4) with ng = 0: r_k = 0 at stage 5, r_k = nu = 4 at stage 2 (there the rows alone fix the gain),
    0..2 elsewhere."""
    from tunempc_amd import convexifier
    A, B, H = gen_batch(5, 3, 8, 6, 4)
    res = convexifier.convexify_batch(A, B, H)
    convexifier.release_handles()
    assert (res['status'] == 0).all()
    rng = np.random.default_rng(7)
    J = rng.standard_normal((3, 8, 4, 10)); ncnt = rng.integers(0, 3, size=(3, 8)).astype(np.int32)
    ncnt[:, 2] = 4; ncnt[:, 5] = 0
    oH = check_parity('(8,6,4) r = 0 .. nu, H from P', A, B, H, J, ncnt, 0, Pi0=res['P'])
    oC = check_parity('(8,6,4) r = 0 .. nu, Hc', A, B, res['Hc'], J, ncnt, 0)
    for b in range(3):
        assert rel(oH['K'][b], oC['K'][b]) <= PARITY
        want = np.linalg.solve(J[b, 2, :, 6:], J[b, 2, :, :6])
        assert rel(oC['K'][b, 2], want) <= PARITY


def test_parity_on_a_block_beyond_32():
    """n = 60 (p 3, nx 40, nu 20) with 2 + 0..3 random rows on the Hc / P of a plain solve: the bordered layout at ld = 65, 89 KB of LDS."""
    from tunempc_amd import convexifier
    A, B, H = gen_batch(11, 2, 3, 40, 20)
    res = convexifier.convexify_batch(A, B, H)
    convexifier.release_handles()
    assert (res['status'] == 0).all()
    J, ncnt = lrr.gen_rows(12, 2, 3, 60, 2, 3)
    check_parity('(3,40,20; 2 + 0..3) H from P', A, B, H, J, ncnt, 2, Pi0=res['P'])
    check_parity('(3,40,20; 2 + 0..3) Hc', A, B, res['Hc'], J, ncnt, 2)


# ----------------------------------------------------------------------------- 5. host entry == device entry; no rows == plain entry
@pytest.mark.parametrize('with_pi0', [False, True])
def test_host_and_device_entries_return_the_same_bits(hc, with_pi0):
    from tunempc_amd import lqr
    A, B, H, J, ncnt, o = step2_solution(hc, 21, 22, 3, 8, 6, 4, 1, 2, 1e-3)
    Hm, p0 = (H, o['P']) if with_pi0 else (o['Hc'], None)
    host = lqr.periodic_lqr_batch(A, B, Hm, Pi0=p0, J=J, ncnt=ncnt, ng=1)
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dev = lqr.periodic_lqr_batch(t(A), t(B), t(Hm), Pi0=t(p0), J=t(J), ncnt=t(ncnt), ng=1)
    assert (host['status'] == 0).all()
    for k in ('K', 'Pi', 'Phi', 'Lam', 'feas', 'info', 'status', 'sweeps'):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda
        np.testing.assert_array_equal(dev[k].cpu().numpy(), host[k], err_msg=k)
    np.testing.assert_array_equal(dev['rho'], host['rho'])
    with pytest.raises(ValueError, match='0 <= ncnt'):
        lqr.periodic_lqr_batch(t(A), t(B), t(Hm), J=t(J), ncnt=t(ncnt) + 5, ng=1)
    with pytest.raises(ValueError, match='one GPU'):
        lqr.periodic_lqr_batch(t(A), t(B), t(Hm), J=torch.from_numpy(J), ng=1)


def test_zero_rows_at_every_stage_return_the_bits_of_the_plain_entry():
    """The bench stage shape and a small one; J with room for rows that no stage uses, and J without any room; host and device entries."""
    from tunempc_amd import lqr
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for (seed, nb, p, nx, mb) in ((7, 3, 64, 24, 8), (11, 8, 1, 4, 2)):
        A, B, H = gen_batch(seed, nb, p, nx, mb)
        plain = lqr.periodic_lqr_batch(A, B, H)
        assert (plain['status'] == 0).all()
        J3 = np.random.default_rng(1).standard_normal((nb, p, 3, nx + mb))
        for J, ncnt, ng in ((J3, np.zeros((nb, p), np.int32), 0), (np.zeros((nb, p, 0, nx + mb)), None, None)):
            for conv in (lambda x: x, t):
                r = lqr.periodic_lqr_batch(conv(A), conv(B), conv(H), J=conv(J), ncnt=conv(ncnt), ng=ng)
                host = (lambda x: x.cpu().numpy()) if conv is t else (lambda x: x)
                for k in ('K', 'Pi', 'Phi', 'info', 'status', 'sweeps'):
                    np.testing.assert_array_equal(host(r[k]), plain[k], err_msg=k)
                np.testing.assert_array_equal(r['rho'], plain['rho'])
                assert not host(r['Lam']).any() and not host(r['feas']).any()


# ----------------------------------------------------------------------------- 6. the certificate after the GPU solve, and the wrong alarm without the rows
def _certify(tag, A, B, H, o, F, J, ncnt, ng):
    from tunempc_amd import lqr
    m = optimal_members(tag, o['status'])
    A, B, H, Hc, P, J, F = (x[m] for x in (A, B, H, o['Hc'], o['P'], J, F))
    ncnt = None if ncnt is None else ncnt[m]
    c = lqr.feedback_equivalence_batch(A, B, H, Hc, P=P, J=J, ncnt=ncnt, ng=ng)
    u = lqr.feedback_equivalence_batch(A, B, H, Hc, P=P)
    mult = F.reshape(len(m), -1).max(axis=1)
    print('%-30s members %d  multipliers %s\n   with rows: dK %s feas %s %s rho %.3g %.3g sweeps %s %s convex_Hc %s\n   without:   dK %s' % (
        tag, len(m), np.round(mult, 3).tolist(), c['dK'].tolist(), c['feas_H'].max(), c['feas_Hc'].max(), c['rho_H'].max(), c['rho_Hc'].max(),
        c['sweeps_H'].tolist(), c['sweeps_Hc'].tolist(), c['convex_Hc'].tolist(), u['dK'].tolist()))
    assert (c['status_H'] == 0).all() and (c['status_Hc'] == 0).all()
    assert (c['dK'] <= PARITY).all()
    assert (c['feas_H'] <= 1e-9).all() and (c['feas_Hc'] <= 1e-9).all()
    assert (c['rho_H'] < 1.0).all() and (c['rho_Hc'] < 1.0).all()
    assert (c['convex_Hc'] == 1.0).all()
    active = mult > 1e-2
    assert active.any(), (tag, mult)                          # without an active multiplier there is no contrast to show
    assert (u['status_H'] == 0).all() and (u['status_Hc'] == 0).all()
    assert (u['dK'][active] > 1e-3).all(), (tag, u['dK'], mult)


def test_certificate_after_step2_and_step1_with_G_at_the_bench_stage_shape(hc):
    """p 64, nx 24, nu 8 with 2 + 0..3 rows, rho = 1e-3 (the batch of test_rows_models_at_the_bench_shape): with the rows dK <= 1e-8, without them the
    unconstrained gains differ by > 1e-3 wherever a multiplier exceeds 1e-2 -- the alarm the certificate gave on these models before it knew the rows."""
    p, nx, mb, nb, ng, nc = 64, 24, 8, 6, 2, 3
    A, B, H = gen_batch(61000, nb, p, nx, mb)
    J, ncnt = lrr.gen_rows(61, nb, p, nx + mb, ng, nc)
    h = hc(p, nx, mb, nb, ng=ng, nc=nc)
    o = h.convexify_step2_batch(A, B, H, J, ncnt, 1e-3)
    _certify('bench shape, Step 2 rho 1e-3', A, B, H, o, o['FgF'], J, ncnt, ng)
    G = np.ascontiguousarray(J[:, :, :ng])
    e = h.convexify_eq_batch(A, B, H, G)
    _certify('bench shape, Step 1 with G', A, B, H, e, e['Fg'], G, None, ng)


def test_certificate_after_step2_at_the_c5_share_shape(hc):
    """p 200, nx 20, nu 10 with 3 + 0..3 rows, rho = 1e-2 (the model of test_rows_models_at_the_c5_share), 8 members."""
    p, nx, mb, nb, ng, nc = 200, 20, 10, 8, 3, 3
    A, B, H = gen_batch(62000, nb, p, nx, mb)
    J, ncnt = lrr.gen_rows(62, nb, p, nx + mb, ng, nc)
    o = hc(p, nx, mb, nb, ng=ng, nc=nc).convexify_step2_batch(A, B, H, J, ncnt, 1e-2)
    _certify('c5 share shape, Step 2 rho 1e-2', A, B, H, o, o['FgF'], J, ncnt, ng)


def test_certificate_with_device_tensors(hc):
    """torch tensors all the way: the device-resident Step 2 solve, then the certificate with the rows on its outputs."""
    from tunempc_amd import lqr
    p, nx, mb, nb, ng, nc = 8, 6, 4, 3, 1, 2
    A, B, H = gen_batch(21, nb, p, nx, mb)
    J, ncnt = lrr.gen_rows(22, nb, p, nx + mb, ng, nc)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dA, dB, dH, dJ, dn = (t(x) for x in (A, B, H, J, ncnt))
    o = hc(p, nx, mb, nb, ng=ng, nc=nc).convexify_con_batch_device(dA, dB, dH, dJ, dn, 1e-3)
    torch.cuda.synchronize()
    assert (o['status'] == 0).all()
    c = lqr.feedback_equivalence_batch(dA, dB, dH, o['Hc'], P=o['P'], J=dJ, ncnt=dn, ng=ng)
    assert isinstance(c['K'], torch.Tensor) and c['K'].is_cuda and isinstance(c['Lam'], torch.Tensor)
    print('device certificate: dK', c['dK'], 'feas', c['feas_H'], c['feas_Hc'])
    assert (c['dK'] <= PARITY).all() and (c['rho_H'] < 1.0).all() and (c['rho_Hc'] < 1.0).all() and (c['convex_Hc'] == 1.0).all()
    assert (c['feas_H'] <= 1e-9).all() and (c['feas_Hc'] <= 1e-9).all()


# ----------------------------------------------------------------------------- 7. through the drop-in
def test_certificate_through_the_dropin_convexify_with_G_and_C():
    """convexify(A, B, Q, R, N, G=, C=) on member 0 of the small Step 2 batch (lists, None where C_k has no row), then the certificate with the same G, C."""
    from tunempc_amd import convexifier, lqr
    p, nx, mb, ng = 8, 6, 4, 1
    A, B, H = gen_batch(21, 3, p, nx, mb)
    J, ncnt = lrr.gen_rows(22, 3, p, nx + mb, ng, 2)
    lst = lambda f: [f(k) for k in range(p)]
    args = (lst(lambda k: A[0, k]), lst(lambda k: B[0, k]), lst(lambda k: H[0, k][:nx, :nx]), lst(lambda k: H[0, k][nx:, nx:]), lst(lambda k: H[0, k][:nx, nx:]))
    G = lst(lambda k: J[0, k, :ng]); C = lst(lambda k: J[0, k, ng:ng + ncnt[0, k]] if ncnt[0, k] else None)
    assert any(c is None for c in C) and any(c is not None and c.shape[0] == 2 for c in C)
    dHc = convexifier.convexify(*args, G=G, C=C)[0]
    convexifier.release_handles()
    c = lqr.feedback_equivalence(*args, dHc, G=G, C=C)
    u = lqr.feedback_equivalence(*args, dHc)
    print('drop-in with G, C: dK %.2e (without the rows %.2e)  feas %.1e %.1e  rho %.3g %.3g  sweeps %d %d' % (
        c['dK'], u['dK'], c['feas_H'], c['feas_Hc'], c['rho_H'], c['rho_Hc'], c['sweeps_H'], c['sweeps_Hc']))
    assert c['status_H'] == 0 and c['status_Hc'] == 0 and c['dK'] <= PARITY and c['rho_H'] < 1.0 and c['rho_Hc'] < 1.0
    assert c['feas_H'] <= 1e-9 and c['feas_Hc'] <= 1e-9 and len(c['K']) == p
    K, Pi, rho = lqr.periodic_lqr(*args[:2], *[[H[0, k][s] + dHc[k][s] for k in range(p)] for s in ((slice(0, nx), slice(0, nx)), (slice(nx, None), slice(nx, None)),
                                                                                             (slice(0, nx), slice(nx, None)))], G=G, C=C)
    assert rel(np.stack(K), np.stack(c['Kc'])) <= PARITY and rho < 1.0
    for k in range(p):
        assert np.abs(G[k][:, :nx] - G[k][:, nx:] @ K[k]).max() <= 1e-9 * max(1.0, np.abs(K[k]).max())


# ----------------------------------------------------------------------------- 8. statuses (return codes of a kernel that finishes)
def test_more_rows_than_inputs_gives_status_4_and_leaves_the_batch_alone():
    """tests/golden/awe_step2_n15.npz (p 40, nx 9, nu 6) has 3 + 4 = 7 rows at several stages: RowsExceedInputs, decided before the first sweep -- sweeps 0, K and
    Lam zero, Pi = Pi0 = 0, Phi and rho NaN.  The member beside it (the same problem with at most one row of C_k per stage) returns what it returns alone."""
    from tunempc_amd import lqr
    g = np.load(os.path.join(GOLDEN, 'awe_step2_n15.npz'))
    J1 = np.concatenate([g['G'], g['C']], axis=2)
    assert J1.shape[2] == 7 and g['B'].shape[3] == 6 and (3 + g['ncnt'] > 6).any()
    two = lambda x: np.concatenate([x, x], axis=0)
    A, B, Hc, J = two(g['A']), two(g['B']), two(g['Hc']), two(J1)
    ncnt = np.concatenate([g['ncnt'], np.minimum(g['ncnt'], 1)], axis=0).astype(np.int32)
    out = lqr.periodic_lqr_batch(A, B, Hc, J=J, ncnt=ncnt, ng=3)
    print('statuses', out['status'], 'sweeps', out['sweeps'], 'info[0]', out['info'][0])
    assert lqr.STATUS_NAMES[int(out['status'][0])] == 'RowsExceedInputs' and int(out['status'][0]) == 4 and int(out['sweeps'][0]) == 0
    assert not out['K'][0].any() and not out['Lam'][0].any() and not out['Pi'][0].any()
    assert np.isnan(out['Phi'][0]).all() and np.isnan(out['rho'][0]) and out['feas'][0] == 0.0
    assert int(out['status'][1]) == 0
    solo = lqr.periodic_lqr_batch(A[1:], B[1:], Hc[1:], J=J[1:], ncnt=ncnt[1:], ng=3)
    for k in ('K', 'Pi', 'Phi', 'Lam', 'info'):
        np.testing.assert_array_equal(out[k][1], solo[k][0], err_msg=k)
    ref = lrr.periodic_lqr(A[1], B[1], Hc[1], J[1], 3 + ncnt[1])
    assert ref['converged'] and rel(out['K'][1], ref['K']) <= PARITY and rel(out['Pi'][1], ref['Pi']) <= PARITY
    with pytest.raises(RuntimeError, match='status 4 \\(RowsExceedInputs\\)'):
        lqr.periodic_lqr([a for a in g['A'][0]], [b for b in g['B'][0]], [h[:9, :9] for h in g['Hc'][0]], [h[9:, 9:] for h in g['Hc'][0]],
                         [h[:9, 9:] for h in g['Hc'][0]], G=[x for x in g['G'][0]], C=[g['C'][0, k, :g['ncnt'][0, k]] if g['ncnt'][0, k] else None for k in range(40)])


def test_two_identical_rows_give_status_2(hc):
    """A repeated row at one stage: Ju loses its row rank, the multiplier pivot vanishes -> status 2 for that member; the others converge as they do alone."""
    from tunempc_amd import lqr
    A, B, H, J, ncnt, o = step2_solution(hc, 21, 22, 3, 8, 6, 4, 1, 2, 1e-3)
    assert (o['status'] == 0).all()
    J = J.copy(); ncnt = ncnt.copy()
    ncnt[1, 3] = max(int(ncnt[1, 3]), 1); J[1, 3, 1] = J[1, 3, 0]                                  # the first row of C_3 repeats the row of G_3
    out = lqr.periodic_lqr_batch(A, B, o['Hc'], J=J, ncnt=ncnt, ng=1)
    print('statuses', out['status'], 'sweeps', out['sweeps'], 'info[1]', out['info'][1])
    assert int(out['status'][1]) == 2 and int(out['sweeps'][1]) == 1 and np.isnan(out['rho'][1]) and out['info'][1, 3] <= 1e-13 * out['info'][1, 4]
    keep = [0, 2]
    solo = lqr.periodic_lqr_batch(A[keep], B[keep], o['Hc'][keep], J=J[keep], ncnt=ncnt[keep], ng=1)
    assert (out['status'][keep] == 0).all()
    for k in ('K', 'Pi', 'Phi', 'Lam', 'info'):
        np.testing.assert_array_equal(out[k][keep], solo[k], err_msg=k)


def test_max_sweeps_gives_status_1_and_a_finite_partial_iterate(hc):
    from tunempc_amd import lqr
    A, B, H, J, ncnt, o = step2_solution(hc, 21, 22, 3, 8, 6, 4, 1, 2, 1e-3)
    assert (o['status'] == 0).all()
    out = lqr.periodic_lqr_batch(A, B, o['Hc'], J=J, ncnt=ncnt, ng=1, max_sweeps=2)
    for b in range(3):
        ref = lrr.periodic_lqr(A[b], B[b], o['Hc'][b], J[b], 1 + ncnt[b], max_sweeps=2)
        assert not ref['converged']
        assert int(out['status'][b]) == 1 and int(out['sweeps'][b]) == 2 and out['info'][b, 2] > 1e-13
        for k in ('K', 'Pi', 'Phi', 'Lam'):
            assert np.isfinite(out[k][b]).all() and rel(out[k][b], ref[k]) <= PARITY, (b, k)
        assert np.isfinite(out['rho'][b]) and out['feas'][b] <= 1e-9 * max(1.0, np.abs(out['K'][b]).max())


# ----------------------------------------------------------------------------- 9. refusals
def test_shapes_beyond_the_lds_and_nr_below_ng_are_refused_with_the_library_message():
    from tunempc_amd import lqr
    A = np.zeros((1, 2, 32, 32)); B = np.zeros((1, 2, 32, 32)); H = np.tile(np.eye(64), (1, 2, 1, 1)); J = np.zeros((1, 2, 40, 64))
    t = lambda x: torch.from_numpy(x).cuda()
    with pytest.raises(NotImplementedError, match='with room for 40 rows per stage needs 183296 bytes of LDS \\(limit 163840\\)'):
        lqr.periodic_lqr_batch(A, B, H, J=J)
    with pytest.raises(NotImplementedError, match='with room for 40 rows per stage needs 183296 bytes of LDS \\(limit 163840\\)'):
        lqr.periodic_lqr_batch(t(A), t(B), t(H), J=t(J))
    with pytest.raises(ValueError, match='0 <= ng <= nr, the row capacity per stage.*ng = 3, nr = 2'):
        lqr.periodic_lqr_batch(A, B, H, J=J[:, :, :2], ng=3)
    with pytest.raises(ValueError, match='0 <= ng <= nr, the row capacity per stage.*ng = 3, nr = 2'):
        lqr.periodic_lqr_batch(t(A), t(B), t(H), J=t(np.ascontiguousarray(J[:, :, :2])), ng=3)
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64 \\(got 65\\)'):
        lqr.periodic_lqr_batch(np.zeros((1, 2, 50, 50)), np.zeros((1, 2, 50, 15)), np.tile(np.eye(65), (1, 2, 1, 1)), J=np.zeros((1, 2, 1, 65)))
