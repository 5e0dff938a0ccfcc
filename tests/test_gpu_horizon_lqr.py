"""GPU tests of the finite-horizon LQR pass (csrc/tmpc_lqr_horizon.h, tunempc_amd.lqr.horizon_*) against the numpy statement in tests/lqr_horizon_reference.py
(SVDs where the kernel eliminates and orthonormalises by Gram-Schmidt), through the host and the device entry.

Every small case runs as a batch of two problems: its H side (indefinite, terminal weight P) and its Hc side (terminal weight zero), so that the grid has more
than one workgroup in both directions and the certificate is checked on the very results that are compared with the reference.

Bounds.  Small cases: the parity bar of this kernel family, 1e-8 relative to max(1, max|.|) of the compared array (test_gpu_ctg_lqr.py).  AWE golden: its own
noise floor, measured by the numpy reference alone in tests/test_lqr_horizon_cpu.py (where the figures are asserted) -- methods (a) and (b) of the reference
disagree by AWE_H_AB_DISAGREEMENT, its two sides by AWE_H_DK, and the bound for K_0 against the reference and for dK0_rel is ten times the larger."""
import functools
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import lqr_horizon_reference as lh  # noqa: E402

PARITY = 1e-8
AWE_H_AB_DISAGREEMENT = 4.7e-10      # measured and asserted in test_lqr_horizon_cpu.py::test_awe_golden_figures_that_bound_the_gpu_test
AWE_H_DK = 6.4e-10
AWE_H_BOUND = 10.0 * max(AWE_H_AB_DISAGREEMENT, AWE_H_DK)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ENTRIES = ['host', 'device']

# (case, terminal, horizons): the synthetic shapes in the modes where they are feasible.  p = 3: N = 1, 2 < p, 3 = p, 4 .. 8 > p; p = 2 and p = 1 likewise
SMALL = [(lh.case_no_rows, 'constraint', (1, 2, 3, 4, 7)), (lh.case_ragged_rows, 'constraint', (1, 2, 3, 4, 5, 8)),
         (lh.case_bench_stage_shape, 'constraint', (1, 8, 9)), (lh.case_ragged_rows, 'cost', (1, 2, 5, 8)),
         (lh.case_bench_stage_shape_ragged, 'cost', (1, 3, 9)), (lh.case_single_phase, 'constraint', (1, 2, 5)), (lh.case_single_phase, 'cost', (1, 2, 5)),
         (lh.case_no_feasible_subspace, 'cost', (1,))]
IDS = ['%s-%s' % (f.__name__, t) for f, t, _ in SMALL]


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def projectors(Hn):
    """Hn [..., nx, nx] (rows beyond c zero) -> Hn' Hn."""
    return np.einsum('...ji,...jl->...il', Hn, Hn)


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def two_sides(case):
    """The batch of two of a case: member 0 its H side with the terminal weight P, member 1 its Hc side with a zero terminal weight."""
    c = case()
    two = lambda x: None if x is None else np.ascontiguousarray(np.concatenate([x, x]))
    return dict(A=two(c['A']), B=two(c['B']), H=np.ascontiguousarray(np.concatenate([c['H'], c['Hc']])), Pf=np.concatenate([c['P'], np.zeros_like(c['P'])]),
                J=two(c['J']), ncnt=two(c['ncnt']), rows=two(c['rows']))


@functools.lru_cache(maxsize=None)
def reference(case, terminal, N, shift=True):
    """The numpy reference of both members of two_sides(case) from all phases, computed once per process and never written to -> [member][phase] dicts."""
    t = two_sides(case)
    return [lh.horizon_lqr_phases(t['A'][b], t['B'][b], t['H'][b], None if t['J'] is None else t['J'][b], t['rows'][b], N, terminal,
                                  t['Pf'][b] if shift else None) for b in range(2)]


def solve(entry, t, N, terminal, members=slice(None), Pf=True, **kw):
    """horizon_lqr_batch on the members of a batch through one entry -> dict of numpy arrays."""
    from tunempc_amd import lqr
    pick = lambda x: None if x is None else np.ascontiguousarray(x[members])
    A, B, H, J, ncnt, Pfm = (pick(t[k]) for k in ('A', 'B', 'H', 'J', 'ncnt', 'Pf'))
    rows = {} if J is None else (dict(J=J) if ncnt is None else dict(J=J, ncnt=ncnt, ng=0))
    if entry == 'host':
        return lqr.horizon_lqr_batch(A, B, H, N, terminal=terminal, Pf=Pfm if Pf else None, **rows, **kw)
    rows = {k: (to_dev(v) if k != 'ng' else v) for k, v in rows.items()}
    out = lqr.horizon_lqr_batch(to_dev(A), to_dev(B), to_dev(H), N, terminal=terminal, Pf=to_dev(Pfm) if Pf else None, **rows, **kw)
    assert all(isinstance(out[k], torch.Tensor) and out[k].is_cuda for k in out if k != 'phases')
    return to_host(out)


def check(tag, out, b, i, r, bound=PARITY):
    """Entry (b, i) of a GPU result against the reference dict r of that (problem, phase): status, c_0, K_0, Pi_0, the feasible subspace, feasibility."""
    nx = r['Pz0'].shape[0]
    e = dict(K0=relmax(out['K0'][b, i], r['K0']), Pi0=relmax(out['Pi0'][b, i], r['Pi0']), Pz0=np.abs(projectors(out['Hn0'][b, i]) - (np.eye(nx) - r['Pz0'])).max())
    print('   %s member %d phase %d: c_0 %d  err %s  feas %.1e  info %s' % (tag, b, i, out['cnt0'][b, i], {k: '%.1e' % v for k, v in e.items()}, out['feas'][b, i],
                                                                      out['info'][b, i].tolist()))
    assert int(out['status'][b, i]) == 0, (tag, b, i, out['info'][b, i])
    assert int(out['cnt0'][b, i]) == int(r['cnt'][0]), (tag, b, i)
    N = r['cnt'].size
    assert out['info'][b, i, 1] == N and out['info'][b, i, 2] == N and out['info'][b, i, 8] == r['cnt'].sum() and out['info'][b, i, 9] == r['cnt'].max()
    assert max(e.values()) <= bound, (tag, b, i, e)
    assert out['feas'][b, i] <= 1e-10 * max(1.0, np.abs(r['K']).max()), (tag, b, i, out['feas'][b, i])
    c = int(r['cnt'][0]); Hn = out['Hn0'][b, i]                                # orthonormal rows, zero beyond c_0
    assert not Hn[c:].any() and (c == 0 or np.abs(Hn[:c] @ Hn[:c].T - np.eye(c)).max() <= 1e-12)


# ----------------------------------------------------------------------------- 1. the small cases, and the certificate read off the same results
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case,terminal,horizons', SMALL, ids=IDS)
def test_small_cases_against_the_reference(entry, case, terminal, horizons):
    t = two_sides(case)
    p = t['A'].shape[1]
    for N in horizons:
        ref = reference(case, terminal, N)
        out = solve(entry, t, N, terminal)
        assert out['K0'].shape[:2] == (2, p) and out['phases'].tolist() == list(range(p))
        for b in range(2):
            for k0 in range(p):
                check('%s %s N %d' % (case.__name__, terminal, N), out, b, k0, ref[b][k0])
        dK = np.abs(out['K0'][0] - out['K0'][1]).max()                        # H side against Hc side
        print('   N %d: dK0 %.1e' % (N, dK))
        assert dK <= PARITY


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case,terminal,N', [(lh.case_ragged_rows, 'constraint', 5), (lh.case_bench_stage_shape, 'constraint', 9),
                                             (lh.case_bench_stage_shape_ragged, 'cost', 9)], ids=['ragged-N5', 'bench-N9', 'bench-ragged-cost-N9'])
def test_return_all_gives_every_stage_of_every_pass(entry, case, terminal, N):
    t = two_sides(case)
    ref = reference(case, terminal, N)
    out = solve(entry, t, N, terminal, return_all=True)
    p = t['A'].shape[1]
    assert out['Kall'].shape == (2, p, N) + ref[0][0]['K0'].shape and out['cntall'].shape == (2, p, N) and out['cntall'].dtype == np.int32
    for b in range(2):
        for k0 in range(p):
            r = ref[b][k0]
            assert out['cntall'][b, k0].tolist() == r['cnt'].tolist(), (b, k0)
            e = max(relmax(out['Kall'][b, k0, j], r['K'][j]) for j in range(N))
            print('   member %d phase %d: cnt %s  worst stage %.1e' % (b, k0, r['cnt'].tolist(), e))
            assert e <= PARITY
            np.testing.assert_array_equal(out['Kall'][b, k0, 0], out['K0'][b, k0])
    plain = solve(entry, t, N, terminal)
    for k in ('K0', 'Pi0', 'Hn0', 'cnt0', 'info'):
        np.testing.assert_array_equal(out[k], plain[k], err_msg=k)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_list_of_phases_is_a_slice_of_the_full_call(entry):
    t = two_sides(lh.case_ragged_rows)
    full = solve(entry, t, 5, 'constraint', return_all=True)
    for phases, sl in (([2], [2]), ([2, 0, 2], [2, 0, 2]), (np.array([1], np.int64), [1])):
        part = solve(entry, t, 5, 'constraint', phases=phases, return_all=True)
        assert part['phases'].tolist() == sl and part['K0'].shape[1] == len(sl)
        for k in ('K0', 'Pi0', 'Hn0', 'cnt0', 'info', 'status', 'feas', 'Kall', 'cntall'):
            np.testing.assert_array_equal(part[k], full[k][:, sl], err_msg=k)


# ----------------------------------------------------------------------------- 2. members and phases do not affect each other
@pytest.mark.parametrize('entry', ENTRIES)
def test_a_poisoned_member_ends_with_status_3_and_leaves_the_others_alone(entry):
    """nb = 3 at the bench stage shape, the middle member with a NaN in H (the xx block of stage 0: found when Pi is formed; the uu block of stage 1: found by
    the pivot search), so that every pass meets one whatever its phase and length."""
    two = two_sides(lh.case_bench_stage_shape)
    t = {k: (None if v is None else np.ascontiguousarray(np.stack([v[0], v[0], v[1]]))) for k, v in two.items()}
    t['H'][1, 0, 0, 0] = np.nan; t['H'][1, 1, 30, 30] = np.nan
    for N in (1, 9):
        out = solve(entry, t, N, 'constraint', return_all=True)
        assert (out['status'][1] == 3).all() and np.isnan(out['K0'][1]).all() and np.isnan(out['Pi0'][1]).all() and not out['Hn0'][1].any()
        assert (out['feas'][1] == 0).all() and np.isnan(out['Kall'][1, :, 0]).all() and (out['cntall'][1, :, 0] == -1).all()
        assert (out['status'][[0, 2]] == 0).all()
        for b, m in ((0, 0), (2, 1)):
            solo = solve(entry, two, N, 'constraint', members=[m], return_all=True)
            for k in ('K0', 'Pi0', 'Hn0', 'cnt0', 'info', 'Kall', 'cntall'):
                np.testing.assert_array_equal(out[k][b], solo[k][0], err_msg=k)


@pytest.mark.parametrize('entry', ENTRIES)
def test_no_feasible_subspace_is_status_5(entry):
    """p 3, nx 4, nu 2, three rows per stage: one state dimension is lost per stage.  N = 4, 7: status 5 at every phase after 3 stages, K0 and Pi0 NaN, Hn0
    zero, cnt0 = nx; N = 1: done with c_0 = 1 (checked against the reference in the small cases)."""
    t = two_sides(lh.case_no_feasible_subspace)
    for N in (4, 7):
        out = solve(entry, t, N, 'cost', return_all=True)
        assert (out['status'] == 5).all() and (out['cnt0'] == 4).all() and (out['info'][..., 2] == 3).all() and (out['feas'] == 0).all()
        assert np.isnan(out['K0']).all() and np.isnan(out['Pi0']).all() and not out['Hn0'].any()
        assert (out['cntall'][..., N - 3:] == [1, 2, 3][::-1]).all() and (out['cntall'][..., :N - 3] == -1).all()
        assert np.isfinite(out['Kall'][:, :, N - 3:]).all() and np.isnan(out['Kall'][:, :, :N - 3]).all()
    out = solve(entry, t, 1, 'cost')
    assert (out['status'] == 0).all() and (out['cnt0'] == 1).all()


# ----------------------------------------------------------------------------- 3. the certificate
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case,terminal,horizons', SMALL, ids=IDS)
def test_certificate_on_the_small_cases(entry, case, terminal, horizons):
    from tunempc_amd import lqr
    c = case()
    f = to_dev if entry == 'device' else (lambda x: x)
    rows = {k: f(v) for k, v in lh.rows_args(c).items()}
    for N in horizons:
        r = lqr.horizon_equivalence_batch(f(c['A']), f(c['B']), f(c['H']), f(c['Hc']), N, P=f(c['P']), terminal=terminal, **rows)
        print('   N %d: dK0 %s  dK0_rel %s  subspace_diff %s  cnt0 %s  feas %s %s' % (N, r['dK0'], r['dK0_rel'], r['subspace_diff'], r['cnt0_H'], r['feas_H'], r['feas_Hc']))
        assert all(isinstance(r[k], np.ndarray) for k in r if k not in ('K0', 'K0c'))
        assert not r['status_H'].any() and not r['status_Hc'].any() and (r['cnt0_H'] == r['cnt0_Hc']).all()
        assert r['dK0'].shape == (1, c['A'].shape[1]) and r['dK0'].max() <= PARITY and r['dK0_rel'].max() <= PARITY and r['subspace_diff'].max() <= PARITY
        assert (r['cnt0_H'][0] == [int(x['cnt'][0]) for x in reference(case, terminal, N)[1]]).all()
    if terminal == 'constraint':                                             # P is optional there: x_N = 0 makes the terminal weight irrelevant
        N = horizons[-1]
        r = lqr.horizon_equivalence_batch(f(c['A']), f(c['B']), f(c['H']), f(c['Hc']), N, terminal=terminal, **rows)
        assert not r['status_H'].any() and r['dK0'].max() <= PARITY


@pytest.mark.parametrize('entry', ENTRIES)
def test_without_the_shift_the_gains_differ(entry):
    """The contrast: both sides with a zero terminal weight (two calls of horizon_lqr_batch with Pf=None) are different problems."""
    t = two_sides(lh.case_ragged_rows)
    d = {}
    for N in (1, 2):
        out = solve(entry, t, N, 'cost', Pf=False)
        ref = reference(lh.case_ragged_rows, 'cost', N, False)
        assert not out['status'].any()
        for b in range(2):
            for k0 in range(3):
                assert relmax(out['K0'][b, k0], ref[b][k0]['K0']) <= PARITY
        d[N] = np.abs(out['K0'][0] - out['K0'][1]).max()
    print(d)
    assert d[1] >= 1e-2 and d[2] >= 1e-2


@functools.lru_cache(maxsize=None)
def awe():
    g = np.load(os.path.join(GOLDEN, 'awe_step2_n15.npz'))
    d = {k: np.ascontiguousarray(g[k], dtype=np.float64) for k in ('A', 'B', 'H', 'Hc', 'P', 'G', 'C')}
    d['ncnt'] = g['ncnt'].astype(np.int32)
    J = np.concatenate([d['G'], d['C']], axis=2)[0]; rows = 3 + d['ncnt'][0]
    d['rH'] = lh.horizon_lqr_phases(d['A'][0], d['B'][0], d['H'][0], J, rows, 20, 'cost', d['P'][0])
    d['rC'] = lh.horizon_lqr_phases(d['A'][0], d['B'][0], d['Hc'][0], J, rows, 20, 'cost', None)
    return d


def test_certificate_on_the_awe_golden():
    """p 40, nx 9, nu 6, 3 + 0..4 rows (7 > 6 at several stages), terminal='cost', N = 20, all 40 phases, through horizon_equivalence in the calling style of
    `convexify` (rows via G= / C=), and the batched call on device tensors: status 0, the c_0 of the reference, equal subspaces, K_0 against the reference and
    dK0_rel within AWE_H_BOUND."""
    from tunempc_amd import lqr
    d = awe()
    rH, rC = d['rH'], d['rC']
    nx, p = 9, 40
    lst = lambda f: [f(k) for k in range(p)]
    H, Hc = d['H'][0], d['Hc'][0]
    args = (lst(lambda k: d['A'][0, k]), lst(lambda k: d['B'][0, k]), lst(lambda k: H[k][:nx, :nx]), lst(lambda k: H[k][nx:, nx:]), lst(lambda k: H[k][:nx, nx:]))
    G = lst(lambda k: d['G'][0, k]); C = lst(lambda k: d['C'][0, k, :d['ncnt'][0, k]] if d['ncnt'][0, k] else None)
    c = lqr.horizon_equivalence(*args, lst(lambda k: Hc[k] - H[k]), 20, P=lst(lambda k: d['P'][0, k]), terminal='cost', G=G, C=C)
    c0 = [int(r['cnt'][0]) for r in rC]
    eH = max(relmax(c['K0'][k], rH[k]['K0']) for k in range(p)); eC = max(relmax(c['K0c'][k], rC[k]['K0']) for k in range(p))
    print('drop-in: dK0_rel %.2e  K0 against the reference %.2e %.2e (bound %.1e)  subspace_diff %.1e  feas %.1e %.1e  c_0 %s' % (
        max(c['dK0_rel']), eH, eC, AWE_H_BOUND, max(c['subspace_diff']), max(c['feas_H']), max(c['feas_Hc']), c['cnt0_H']))
    assert not any(c['status_H']) and not any(c['status_Hc']) and c['cnt0_H'] == c0 and c['cnt0_Hc'] == c0 and c['phases'] == list(range(p))
    assert max(c['subspace_diff']) <= PARITY and max(c['feas_H']) <= 1e-10 * 37.7 and max(c['feas_Hc']) <= 1e-10 * 37.7
    assert eH <= AWE_H_BOUND and eC <= AWE_H_BOUND and max(c['dK0_rel']) <= AWE_H_BOUND
    K0, Pi0, cnt0 = lqr.horizon_lqr(*args, 20, terminal='cost', Pf=lst(lambda k: d['P'][0, k]), G=G, C=C)
    assert cnt0 == c0 and max(relmax(K0[k], rH[k]['K0']) for k in range(p)) <= AWE_H_BOUND
    assert max(relmax(Pi0[k], rH[k]['Pi0']) for k in range(p)) <= AWE_H_BOUND
    t = to_dev
    cd = lqr.horizon_equivalence_batch(t(d['A']), t(d['B']), t(d['H']), t(d['Hc']), 20, P=t(d['P']), terminal='cost', J=t(np.concatenate([d['G'], d['C']], axis=2)),
                                       ncnt=t(d['ncnt']), ng=3)
    assert not cd['status_H'].any() and cd['cnt0_H'][0].tolist() == c0 and cd['dK0_rel'].max() <= AWE_H_BOUND
    np.testing.assert_array_equal(cd['K0'].cpu().numpy()[0], np.stack(c['K0']))


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_long_horizon_gives_the_periodic_gain(entry):
    """p 3, nx 3, nu 2 with a terminal constraint at N = 24 against the GPU's own periodic gains (the constraint-to-go entry), both members; at N = 6 they differ."""
    from tunempc_amd import lqr
    t = two_sides(lh.case_ragged_rows)
    f = to_dev if entry == 'device' else (lambda x: x)
    per = to_host(lqr.periodic_lqr_batch(f(t['A']), f(t['B']), f(t['H']), Pi0=f(t['Pf']), J=f(t['J']), ncnt=f(t['ncnt']), ng=0, state_rows=True))
    assert not per['status'].any() and not per['cnt'].any()
    d = {N: np.abs(solve(entry, t, N, 'constraint')['K0'] - per['K']).max() for N in (6, 24)}
    print(d, per['rho'])
    assert d[24] <= PARITY and d[6] >= 1e-6


# ----------------------------------------------------------------------------- 4. refusals
def test_shapes_beyond_the_layout_are_refused_before_a_launch():
    from tunempc_amd import lqr
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='nx = 32, nu = 32 with room for 40 rows per stage and a constraint-to-go needs \\d+ bytes of LDS'):
        lqr.horizon_lqr_batch(z(1, 2, 32, 32), z(1, 2, 32, 32), z(1, 2, 64, 64), 3, J=z(1, 2, 40, 64))
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64'):
        lqr.horizon_lqr_batch(np.zeros((1, 2, 40, 40)), np.zeros((1, 2, 40, 30)), np.zeros((1, 2, 70, 70)), 3)
    with pytest.raises(ValueError, match='phases must lie in 0 .. p - 1 = 1'):
        lqr.horizon_lqr_batch(z(1, 2, 3, 3), z(1, 2, 3, 1), z(1, 2, 4, 4), 3, phases=[2])
