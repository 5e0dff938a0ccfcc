"""GPU tests of the constraint-to-go recursion (csrc/tmpc_lqr_ctg.h, the state_rows= / rank_tol= arguments of tunempc_amd/lqr.py) against the numpy statement in
tests/lqr_ctg_reference.py (SVDs where the kernel eliminates and orthonormalises by Gram-Schmidt), through the host and the device entry.

Bounds.  Small cases: the parity bar of this kernel family, 1e-8 relative to max(1, max|.|) of the compared array.  AWE golden: its own noise floor, measured by
the numpy reference alone in tests/test_lqr_ctg_cpu.py (where the figures are asserted) -- methods (a) and (b) of the reference disagree by AWE_AB_DISAGREEMENT,
five further sweeps of (a) move its outputs by AWE_WOBBLE, and the bound for K, Pi, Phi against the reference and for dK is ten times the larger."""
import functools
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_ctg_reference as lc  # noqa: E402

PARITY = 1e-8
AWE_AB_DISAGREEMENT = 2.7e-11        # measured and asserted in test_lqr_ctg_cpu.py::test_awe_golden_certificate_and_the_figures_that_bound_the_gpu_test
AWE_WOBBLE = 5.2e-11
AWE_BOUND = 10.0 * max(AWE_AB_DISAGREEMENT, AWE_WOBBLE)
AWE_TOL = 1e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def projectors(Hn):
    """Hn [..., nx, nx] (rows beyond c zero) -> Hn' Hn."""
    return np.einsum('...ji,...jl->...il', Hn, Hn)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The numpy reference of one small case, computed once per process and never written to."""
    A, B, H, J, ncnt = case()[:5]
    return lc.periodic_lqr_batch(A, B, H, J, ncnt, tol=lc.TOL)


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def solve(entry, A, B, H, J, ncnt, **kw):
    from tunempc_amd import lqr
    kw.setdefault('tol', lc.TOL)
    if entry == 'host':
        return lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt, ng=0, state_rows=True, **kw)
    kw = {k: (to_dev(v) if k == 'Pi0' else v) for k, v in kw.items()}
    out = lqr.periodic_lqr_batch(to_dev(A), to_dev(B), to_dev(H), J=to_dev(J), ncnt=to_dev(ncnt), ng=0, state_rows=True, **kw)
    assert all(isinstance(out[k], torch.Tensor) and out[k].is_cuda for k in ('K', 'Pi', 'Phi', 'Hn', 'cnt', 'feas', 'info', 'status', 'sweeps'))
    return to_host(out)


def check_member(tag, out, b, r, bound=PARITY):
    """Member b of a GPU result against its reference dict r: status, counts, K, Pi, Phi, the feasible subspaces, feasibility, rho."""
    e = dict(K=relmax(out['K'][b], r['K']), Pi=relmax(out['Pi'][b], r['Pi']), Phi=relmax(out['Phi'][b], r['Phi']),
             Pz=np.abs(projectors(out['Hn'][b]) - (np.eye(r['Pz'].shape[1]) - r['Pz'])).max())
    print('   %s member %d: sweeps gpu %d numpy %d  cnt %s  err %s  feas %.1e  info %s' % (
        tag, b, out['sweeps'][b], r['sweeps'], out['cnt'][b].tolist(), {k: '%.1e' % v for k, v in e.items()}, out['feas'][b], out['info'][b].tolist()))
    assert int(out['status'][b]) == 0, (tag, b, out['info'][b])
    assert out['cnt'][b].tolist() == r['cnt'].tolist(), (tag, b)
    assert out['info'][b, 8] == r['cnt'].sum() and out['info'][b, 9] == r['cnt'].max()
    assert e['K'] <= bound and e['Pi'] <= bound and e['Phi'] <= bound and e['Pz'] <= PARITY, (tag, b, e)
    assert out['feas'][b] <= 1e-10 * max(1.0, np.abs(r['K']).max()), (tag, b, out['feas'][b])
    assert abs(out['rho'][b] - r['rho']) <= PARITY * max(1.0, r['rho'])
    for k in range(r['cnt'].size):                                            # orthonormal rows, zero beyond c_k
        c = int(r['cnt'][k]); N = out['Hn'][b, k]
        assert not N[c:].any() and np.abs(N[:c] @ N[:c].T - np.eye(c)).max() <= 1e-12 if c else not N.any()
    if out['info'][b, 8] > 0:                                                 # the rank decisions were clear-cut
        assert out['info'][b, 10] >= lc.ACCEPT_MIN
    assert out['info'][b, 11] <= 10.0 * lc.REJECT_MAX                                # (one decade over the reference's own limit for the growth of the elimination)


ENTRIES = ['host', 'device']


# ----------------------------------------------------------------------------- 1. the smallest leftover row
@pytest.mark.parametrize('entry', ENTRIES)
def test_one_stage_with_two_rows_and_one_input(entry):
    A, B, H, J, ncnt = lc.case_leftover_row()
    out = solve(entry, A, B, H, J, ncnt)
    assert out['cnt'][0].tolist() == [0, 1, 0]
    assert 'Lam' not in out and out['info'].shape == (1, 12)
    check_member('leftover row', out, 0, reference(lc.case_leftover_row)[0])


# ----------------------------------------------------------------------------- 2. the constraint wraps onto itself
@pytest.mark.parametrize('entry', ENTRIES)
def test_no_feasible_subspace_is_status_5_and_leaves_the_batch_alone(entry):
    from tunempc_amd import lqr
    A, B, H, J, ncnt = lc.case_wrap_onto_itself()
    out = solve(entry, A, B, H, J, ncnt)
    ref = reference(lc.case_wrap_onto_itself)
    print('statuses', out['status'], 'sweeps', out['sweeps'], 'info[0]', out['info'][0])
    assert ref[0]['infeasible']
    assert int(out['status'][0]) == 5 and lqr.STATUS_NAMES[5] == 'NoFeasibleSubspace' and int(out['sweeps'][0]) <= 3
    assert np.isnan(out['Phi'][0]).all() and np.isnan(out['rho'][0]) and out['feas'][0] == 0.0
    solo = solve(entry, A[1:], B[1:], H[1:], J[1:], ncnt[1:])
    for b in (1, 2):
        check_member('beside status 5', out, b, ref[b])
        for k in ('K', 'Pi', 'Phi', 'Hn', 'cnt', 'info'):
            np.testing.assert_array_equal(out[k][b], solo[k][b - 1], err_msg=k)


# ----------------------------------------------------------------------------- 3. a row on the state alone
@pytest.mark.parametrize('entry', ENTRIES)
def test_a_state_only_row(entry):
    from tunempc_amd import lqr
    A, B, H, J, ncnt = lc.case_state_only_row()
    assert not J[0, 2, 0, 4:].any() and ncnt[0, 2] == 2
    out = solve(entry, A, B, H, J, ncnt)
    assert int(out['status'][0]) == 0 and out['cnt'][0, 2] >= 1
    check_member('state-only row', out, 0, reference(lc.case_state_only_row)[0])
    plain = lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt, ng=0, tol=lc.TOL)
    assert int(plain['status'][0]) == 2                                       # what the call answers without state_rows stays as it was


# ----------------------------------------------------------------------------- 4. a duplicated row
@pytest.mark.parametrize('entry', ENTRIES)
def test_a_duplicated_row_is_dropped(entry):
    from tunempc_amd import lqr
    A, B, H, J, ncnt, ncnt1 = lc.case_duplicated_row()
    assert (ncnt <= 2).all() and (J[0, 1, 1] == 2.0 * J[0, 1, 0]).all()
    plain = lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt, ng=0, tol=lc.TOL)
    assert int(plain['status'][0]) == 2
    out = solve(entry, A, B, H, J, ncnt)
    check_member('duplicated row', out, 0, reference(lc.case_duplicated_row)[0])
    without = lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt1, ng=0, tol=lc.TOL)      # the rows entry on the problem without the duplicate
    assert int(without['status'][0]) == 0
    assert relmax(out['K'], without['K']) <= PARITY and relmax(out['Pi'], without['Pi']) <= PARITY and not out['cnt'].any()


# ----------------------------------------------------------------------------- 5. counts that accumulate; batch independence
@pytest.mark.parametrize('entry', ENTRIES)
def test_counts_accumulate_over_consecutive_stages_and_members_do_not_mix(entry):
    A, B, H, J, ncnt = lc.case_accumulating()
    out = solve(entry, A, B, H, J, ncnt)
    ref = reference(lc.case_accumulating)
    for b in range(5):
        assert out['cnt'][b].tolist() == [0, 1, 3, 2, 1, 0]
        check_member('accumulating', out, b, ref[b])
        solo = solve(entry, A[b:b + 1], B[b:b + 1], H[b:b + 1], J[b:b + 1], ncnt[b:b + 1])
        for k in ('K', 'Pi', 'Phi', 'Hn', 'cnt', 'info', 'feas'):
            np.testing.assert_array_equal(out[k][b], solo[k][0], err_msg=k)


# ----------------------------------------------------------------------------- 6. rows within the inputs: the rows entry
@pytest.mark.parametrize('entry', ENTRIES)
def test_with_rows_that_fit_the_inputs_it_agrees_with_the_rows_entry(entry):
    from tunempc_amd import lqr
    A, B, H, J, ncnt = lc.case_rows_within_inputs()
    out = solve(entry, A, B, H, J, ncnt)
    rows = lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt, ng=0, tol=lc.TOL)
    ref = reference(lc.case_rows_within_inputs)
    assert (rows['status'] == 0).all() and not out['cnt'].any()
    for b in range(A.shape[0]):
        check_member('rows within inputs', out, b, ref[b])
        e = {k: relmax(out[k][b], rows[k][b]) for k in ('K', 'Pi', 'Phi')}
        print('   against the rows entry', b, e, 'sweeps', out['sweeps'][b], rows['sweeps'][b])
        assert max(e.values()) <= 1e-12, (b, e)


# ----------------------------------------------------------------------------- 7. the bench stage shape: the wide layout
@pytest.mark.parametrize('entry', ENTRIES)
def test_the_bench_stage_shape_with_9_and_10_rows(entry):
    A, B, H, J, ncnt = lc.case_bench_stage_shape()
    assert A.shape == (4, 8, 24, 24) and B.shape[3] == 8 and sorted(set(ncnt[0].tolist())) == [5, 9, 10]
    out = solve(entry, A, B, H, J, ncnt)
    ref = reference(lc.case_bench_stage_shape)
    for b in range(4):
        assert out['cnt'][b].tolist() == [0, 0, 2, 0, 0, 1, 0, 0]
        check_member('bench stage shape', out, b, ref[b])


# ----------------------------------------------------------------------------- 8. the certificate on the AWE golden
@functools.lru_cache(maxsize=None)
def awe():
    g = np.load(os.path.join(GOLDEN, 'awe_step2_n15.npz'))
    d = {k: np.ascontiguousarray(g[k], dtype=np.float64) for k in ('A', 'B', 'H', 'Hc', 'P', 'G', 'C')}
    d['ncnt'] = g['ncnt'].astype(np.int32)
    J = np.concatenate([d['G'], d['C']], axis=2)[0]; rows = 3 + d['ncnt'][0]
    d['rH'] = lc.periodic_lqr(d['A'][0], d['B'][0], d['H'][0], J, rows, Pi0=d['P'][0], tol=AWE_TOL)
    d['rC'] = lc.periodic_lqr(d['A'][0], d['B'][0], d['Hc'][0], J, rows, tol=AWE_TOL)
    return d


def test_certificate_on_the_awe_golden():
    """p 40, nx 9, nu 6, 3 + 0..4 rows (7 > 6 at several stages): through feedback_equivalence in the calling style of `convexify`, and the batched call
    on device tensors.  Status 0 on both sides, the counts of the reference, equal subspaces, rho < 1, feas <= 1e-10, K / Pi / Phi against the reference and
    dK within AWE_BOUND; without state_rows the same call answers status 4."""
    from tunempc_amd import lqr
    d = awe()
    rH, rC = d['rH'], d['rC']
    assert rH['converged'] and rC['converged'] and (rH['cnt'] == rC['cnt']).all() and rH['cnt'].sum() == 12
    nx, p = 9, 40
    lst = lambda f: [f(k) for k in range(p)]
    H, Hc = d['H'][0], d['Hc'][0]
    args = (lst(lambda k: d['A'][0, k]), lst(lambda k: d['B'][0, k]), lst(lambda k: H[k][:nx, :nx]), lst(lambda k: H[k][nx:, nx:]), lst(lambda k: H[k][:nx, nx:]))
    G = lst(lambda k: d['G'][0, k]); C = lst(lambda k: d['C'][0, k, :d['ncnt'][0, k]] if d['ncnt'][0, k] else None)
    dHc = lst(lambda k: Hc[k] - H[k])
    c = lqr.feedback_equivalence(*args, dHc, tol=AWE_TOL, G=G, C=C, state_rows=True)
    kmax = max(1.0, np.abs(rC['K']).max())
    print('drop-in: dK %.2e (of max|K|: %.2e, bound %.1e)  subspace_diff %.1e  feas %.1e %.1e  rho %.3g %.3g  sweeps %d %d  cnt %s' % (
        c['dK'], c['dK'] / kmax, AWE_BOUND, c['subspace_diff'], c['feas_H'], c['feas_Hc'], c['rho_H'], c['rho_Hc'], c['sweeps_H'], c['sweeps_Hc'], c['cnt']))
    assert c['status_H'] == 0 and c['status_Hc'] == 0
    assert c['cnt'] == rH['cnt'].tolist() and c['cntc'] == rC['cnt'].tolist()
    assert c['subspace_diff'] <= 1e-12 and c['rho_H'] < 1.0 and c['rho_Hc'] < 1.0 and c['feas_H'] <= 1e-10 and c['feas_Hc'] <= 1e-10
    assert np.isfinite(c['dK']) and c['dK'] / kmax <= AWE_BOUND and c['dK_rel'] <= AWE_BOUND
    eK = max(relmax(np.stack(c['K']), rH['K']), relmax(np.stack(c['Kc']), rC['K']))
    print('K against the reference: %.2e' % eK)
    assert eK <= AWE_BOUND
    # the batched certificate with the P of the file (H side from Pi0 = P), host entry
    J = np.concatenate([d['G'], d['C']], axis=2)
    cb = lqr.feedback_equivalence_batch(d['A'], d['B'], d['H'], d['Hc'], P=d['P'], tol=AWE_TOL, J=J, ncnt=d['ncnt'], ng=3, state_rows=True)
    print('batched, from P: dK %.2e (of max|K|: %.2e)  subspace_diff %.1e  feas %.1e %.1e  rho %.3g %.3g  sweeps %d %d' % (
        cb['dK'][0], cb['dK'][0] / kmax, cb['subspace_diff'][0], cb['feas_H'][0], cb['feas_Hc'][0], cb['rho_H'][0], cb['rho_Hc'][0], cb['sweeps_H'][0], cb['sweeps_Hc'][0]))
    assert cb['status_H'][0] == 0 and cb['status_Hc'][0] == 0 and cb['cnt'][0].tolist() == rH['cnt'].tolist() and cb['cntc'][0].tolist() == rC['cnt'].tolist()
    assert cb['subspace_diff'][0] <= 1e-12 and cb['rho_H'][0] < 1.0 and cb['rho_Hc'][0] < 1.0 and cb['feas_H'][0] <= 1e-10 and cb['feas_Hc'][0] <= 1e-10
    assert np.isfinite(cb['dK'][0]) and cb['dK'][0] / kmax <= AWE_BOUND
    assert relmax(cb['K'][0], rH['K']) <= AWE_BOUND and relmax(cb['Kc'][0], rC['K']) <= AWE_BOUND
    ub = lqr.feedback_equivalence_batch(d['A'], d['B'], d['H'], d['Hc'], P=d['P'], tol=AWE_TOL, J=J, ncnt=d['ncnt'], ng=3)
    assert ub['status_H'][0] == 4 and ub['status_Hc'][0] == 4
    # the batched call on device tensors: the certificate, then each side against its reference
    t = to_dev
    cd = lqr.feedback_equivalence_batch(t(d['A']), t(d['B']), t(d['H']), t(d['Hc']), P=t(d['P']), tol=AWE_TOL, J=t(J), ncnt=t(d['ncnt']), ng=3, state_rows=True)
    assert isinstance(cd['Hn'], torch.Tensor) and cd['Hn'].is_cuda and cd['subspace_diff'][0] <= 1e-12
    assert cd['dK'][0] == cb['dK'][0] and cd['cnt'].cpu().numpy().tolist() == cb['cnt'].tolist()
    for side, Hm, P0, r in (('H', d['H'], d['P'], rH), ('Hc', d['Hc'], None, rC)):
        o = to_host(lqr.periodic_lqr_batch(t(d['A']), t(d['B']), t(Hm), Pi0=t(P0), tol=AWE_TOL, J=t(J), ncnt=t(d['ncnt']), ng=3, state_rows=True))
        check_member('AWE ' + side, o, 0, r, bound=AWE_BOUND)
    u = lqr.feedback_equivalence(*args, dHc, tol=AWE_TOL, G=G, C=C)
    assert u['status_H'] == 4 and u['status_Hc'] == 4
    with pytest.raises(RuntimeError, match='status 4 \\(RowsExceedInputs\\)'):
        lqr.periodic_lqr(*args, tol=AWE_TOL, G=G, C=C)
    K, Pi, rho = lqr.periodic_lqr(*args, tol=AWE_TOL, G=G, C=C, state_rows=True)
    assert relmax(np.stack(K), rH['K']) <= AWE_BOUND and rho < 1.0


# ----------------------------------------------------------------------------- 9. the default call is the rows entry
def test_without_state_rows_the_call_returns_the_bits_of_the_rows_entry():
    from tunempc_amd import _lib, lqr
    A, B, H, J, ncnt = lc.case_rows_within_inputs()
    out = lqr.periodic_lqr_batch(A, B, H, J=J, ncnt=ncnt, ng=0)
    K, Pi, Phi, Lam, info = _lib.periodic_lqr_rows_batch_host(A, B, H, J, ncnt, 0, None, 1e-13, 5000)
    for k, v in (('K', K), ('Pi', Pi), ('Phi', Phi), ('Lam', Lam), ('info', info)):
        np.testing.assert_array_equal(out[k], v, err_msg=k)
    assert 'Hn' not in out and 'cnt' not in out and out['info'].shape[1] == 8
    c = lqr.feedback_equivalence_batch(A, B, H, H, J=J, ncnt=ncnt, ng=0)
    assert 'subspace_diff' not in c and 'Lam' in c
