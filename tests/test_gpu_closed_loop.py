"""GPU tests of the closed-loop rollout (csrc/tmpc_closed_loop.h, tunempc_amd.closed_loop) against the numpy loop in tests/closed_loop_reference.py, through
the host and the device entry.

Bounds.  Against the reference: the parity bar of this kernel family, 1e-8 relative to max(1, max|.|) of the compared array.  Bit-identity where the kernel
promises it (a state alone against the same state in a tile, the two entries, an absent input, return_traj=False).  The telescoping identity: ten times the
figure the numpy reference reaches by itself (test_closed_loop_cpu.py, where it is asserted), or the accuracy at which the solver returned dHc against its own
P, whichever is larger."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import closed_loop_reference as cr  # noqa: E402
import lqr_horizon_reference as lh  # noqa: E402
from test_closed_loop_cpu import TELESCOPING_DEFECT_REL, RHO_RAGGED  # noqa: E402

PARITY = 1e-8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ENTRIES = ['host', 'device']
STEP_KEYS = ('l', 'lc', 'rowres', 'subres')
ALL_KEYS = ('X', 'U') + STEP_KEYS + ('XT', 'L', 'Lc', 'status', 'steps', 'xmax', 'info')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def to_dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def run(entry, d, T, k0=0, use=('H', 'Hc', 'J', 'Hn'), states=slice(None), members=slice(None), **kw):
    """closed_loop_batch on (a slice of) the batch d through one entry -> dict of numpy arrays (None for what is absent)."""
    from tunempc_amd import closed_loop as cl
    pick = lambda x: None if x is None else np.ascontiguousarray(x[members])
    f = to_dev if entry == 'device' else (lambda x: x)
    opt = {k: f(pick(d[k])) for k in ('H', 'Hc', 'Hn') if k in use and d.get(k) is not None}
    if 'J' in use and d.get('J') is not None:
        opt['J'] = f(pick(d['J']))
        if d.get('ncnt') is not None:
            opt.update(ncnt=f(pick(d['ncnt'])), ng=0)
    out = cl.closed_loop_batch(f(pick(d['A'])), f(pick(d['B'])), f(pick(d['K'])), f(np.ascontiguousarray(pick(d['X0'])[:, states])), T, k0, **opt, **kw)
    if entry == 'device':
        assert all(v is None or (isinstance(v, torch.Tensor) and v.is_cuda) for v in out.values())
    return to_host(out)


def as_batch(d):
    """A case of closed_loop_reference.with_feedback (one problem) as a batch of one."""
    return {k: (None if v is None else np.ascontiguousarray(v[None])) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def small(name):
    """(batch, T, phase0) of the smallest shapes, built once and never written to."""
    if name == 'one':                       # (nb, p, nx, nu, ns, T) = (1, 1, 1, 1, 1, 1)
        return cr.random_batch(3, 1, 1, 1, 1, 1, nr=1), 1, 0
    if name == 'wrap':                      # T is no multiple of p and the phase wraps; ragged rows 1, 0, 2
        return cr.random_batch(4, 2, 3, 3, 2, 5, nr=2, ncnt=[1, 0, 2]), 7, 2
    if name == 'p1':
        return cr.random_batch(5, 2, 1, 3, 2, 3, nr=1), 4, 0
    if name == 'bench-ragged':              # nx 24 / nu 8, p = 2, rows 5 / 3
        return as_batch(cr.with_feedback(lh.case_bench_stage_shape_ragged, ns=3)), 5, 1
    if name == 'n64':                       # nx 40 / nu 24: TS = 32
        return cr.random_batch(6, 1, 2, 40, 24, 3, nr=3, ncnt=[3, 1]), 2, 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def small_reference(name):
    d, T, k0 = small(name)
    opt = lambda k, b: None if d.get(k) is None else d[k][b]
    return [cr.rollout(d['A'][b], d['B'][b], d['K'][b], d['X0'][b], T, k0, H=opt('H', b), Hc=opt('Hc', b), J=opt('J', b), rows=opt('rows', b), Hn=opt('Hn', b))
            for b in range(d['A'].shape[0])]


# ----------------------------------------------------------------------------- 1. the smallest shapes against the reference
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', ['one', 'wrap', 'p1', 'bench-ragged', 'n64'])
def test_smallest_shapes_against_the_reference(entry, name):
    d, T, k0 = small(name)
    ref = small_reference(name)
    out = run(entry, d, T, k0)
    nb, ns = d['X0'].shape[:2]
    assert out['X'].shape == (nb, ns, T + 1) + d['X0'].shape[2:] and out['U'].shape == (nb, ns, T, d['B'].shape[3]) and out['l'].shape == (nb, ns, T)
    assert out['status'].dtype == np.int32 and not out['status'].any() and (out['steps'] == T).all() and (out['info'][..., 3] == 0).all()
    for b in range(nb):
        e = {k: relmax(out[k][b], ref[b][k]) for k in ('X', 'U', 'XT', 'L', 'Lc') + STEP_KEYS}
        print('   %s %s member %d: %s' % (name, entry, b, {k: '%.1e' % v for k, v in e.items()}))
        assert max(e.values()) <= PARITY, e
        np.testing.assert_array_equal(out['X'][b, :, 0], d['X0'][b])
        np.testing.assert_array_equal(out['X'][b, :, T], out['XT'][b])
        assert relmax(out['xmax'][b], np.abs(ref[b]['X']).max(axis=(1, 2))) <= PARITY
    np.testing.assert_array_equal(out['info'][..., 0], out['status']); np.testing.assert_array_equal(out['info'][..., 2], out['xmax'])
    short = run(entry, d, T, k0, return_traj=False)
    assert short['X'] is None and short['U'] is None
    for k in ALL_KEYS[2:]:
        np.testing.assert_array_equal(short[k], out[k], err_msg=k)


# ----------------------------------------------------------------------------- 2. tile edges: a state's numbers do not depend on its neighbours
@functools.lru_cache(maxsize=None)
def tile_case(name):
    from tunempc_amd import closed_loop as cl
    nx, mb, nr, p, T = {'ts64': (3, 2, 2, 3, 4), 'ts32': (40, 24, 1, 2, 2)}[name]
    ts = cl.lds_layout(nx, mb, nr)['ts']
    assert ts == {'ts64': 64, 'ts32': 32}[name]
    d = cr.random_batch(8, 1, p, nx, mb, ts + 1, nr=nr)
    solo = [run('device', d, T, 1, states=slice(s, s + 1)) for s in range(ts + 1)]      # every state launched alone, once
    return d, T, ts, solo


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', ['ts64', 'ts32'])
def test_tile_edges_are_bit_identical_to_the_states_alone(entry, name):
    d, T, ts, solo = tile_case(name)
    for ns in (ts - 1, ts, ts + 1):
        out = run(entry, d, T, 1, states=slice(0, ns))
        assert not out['status'].any()
        for s in range(ns):
            for k in ALL_KEYS:
                np.testing.assert_array_equal(out[k][:, s], solo[s][k][:, 0], err_msg='%s ns %d state %d' % (k, ns, s))
    ref = cr.rollout(d['A'][0], d['B'][0], d['K'][0], d['X0'][0], T, 1, H=d['H'][0], Hc=d['Hc'][0], J=d['J'][0], Hn=d['Hn'][0])
    assert max(relmax(out[k][0], ref[k]) for k in ('X', 'U', 'XT') + STEP_KEYS) <= PARITY      # (the last call: ns = TS + 1, two tiles)


# ----------------------------------------------------------------------------- 3. optional inputs
@pytest.mark.parametrize('entry', ENTRIES)
def test_an_absent_input_changes_no_other_output(entry):
    d, T, k0 = small('wrap')
    full = run(entry, d, T, k0)
    need = dict(l='H', lc='Hc', rowres='J', subres='Hn', L='H', Lc='Hc')
    for r in range(5):
        for use in itertools.combinations(('H', 'Hc', 'J', 'Hn'), r):
            out = run(entry, d, T, k0, use=use)
            for k in ALL_KEYS:
                if k in need and need[k] not in use:
                    assert out[k] is None, (use, k)
                else:
                    np.testing.assert_array_equal(out[k], full[k], err_msg='%s with %s' % (k, use))


# ----------------------------------------------------------------------------- 4. the monodromy of the periodic gains
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('mode', ['plain', 'rows', 'state_rows'])
@pytest.mark.parametrize('case', [lh.case_ragged_rows, lh.case_bench_stage_shape_ragged], ids=['ragged', 'bench-ragged'])
def test_monodromy_reproduces_the_periodic_call(entry, mode, case):
    from tunempc_amd import closed_loop as cl, lqr
    c = case()
    f = to_dev if entry == 'device' else (lambda x: x)
    A, B, Hc = f(c['A']), f(c['B']), f(c['Hc'])
    rows = {} if mode == 'plain' else dict(J=f(c['J']), ncnt=f(c['ncnt']), ng=0)
    if mode == 'state_rows':
        rows['state_rows'] = True
    per = lqr.periodic_lqr_batch(A, B, Hc, **rows)
    assert not to_host(per)['status'].any()
    Pz0 = None
    if mode == 'state_rows':
        Hn0 = per['Hn'][:, 0]
        Pz0 = f(np.eye(c['A'].shape[2])[None]) - (Hn0.transpose(1, 2) if entry == 'device' else Hn0.transpose(0, 2, 1)) @ Hn0
    m = cl.closed_loop_monodromy_batch(A, B, per['K'], Pz0=Pz0)
    Phi, want = to_host(m)['Phi'], to_host(per)['Phi']
    e = relmax(Phi, want)
    print('   %s %s %s: Phi %.2e  rho %.12f against %.12f' % (case.__name__, mode, entry, e, m['rho'][0], per['rho'][0]))
    assert e <= PARITY and abs(m['rho'][0] - per['rho'][0]) <= PARITY * max(1.0, per['rho'][0]) and not m['status'].any()
    assert isinstance(m['rho'], np.ndarray) and m['Phi'].shape == per['Phi'].shape


# ----------------------------------------------------------------------------- 5. the receding-horizon loop
@functools.lru_cache(maxsize=None)
def receding_reference(N):
    c = lh.case_ragged_rows()
    return cr.receding_horizon(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], N, 'cost', None)


@pytest.mark.parametrize('entry', ENTRIES)
def test_receding_horizon_scan(entry):
    from tunempc_amd import closed_loop as cl, lqr
    c = lh.case_ragged_rows()
    f = to_dev if entry == 'device' else (lambda x: x)
    Ns = (1, 2, 5, 8, 30)
    rows = dict(J=f(c['J']), ncnt=f(c['ncnt']), ng=0)
    r = cl.horizon_closed_loop_batch(f(c['A']), f(c['B']), f(c['Hc']), Ns, terminal='cost', **rows)
    print('   rho %s  subres %s  status %s' % (r['rho'], r['subres'], r['status']))
    assert r['rho'].shape == (1, 5) and r['Phi'].shape == (1, 5, 3, 3) and not r['status'].any() and r['horizons'].tolist() == list(Ns)
    for i, N in enumerate(Ns):
        ref = receding_reference(N)
        assert abs(r['rho'][0, i] - ref['rho']) <= PARITY and abs(ref['rho'] - RHO_RAGGED[N]) <= 5e-4 * RHO_RAGGED[N]
        assert relmax(to_host(dict(P=r['Phi']))['P'][0, i], ref['Phi']) <= PARITY
        assert r['subres'][0, i] <= 1e-10                                     # the law keeps the state on the next phase's feasible set
    per = lqr.periodic_lqr_batch(f(c['A']), f(c['B']), f(c['Hc']), state_rows=True, **rows)
    assert not to_host(per)['status'].any()
    print('   periodic rho %.12f' % per['rho'][0])
    assert abs(r['rho'][0, 4] - per['rho'][0]) <= 1e-6 and abs(r['rho'][0, 3] - per['rho'][0]) <= 1e-5
    assert (np.diff(r['rho'][0]) < 0).all()


@pytest.mark.parametrize('entry', ENTRIES)
def test_receding_horizon_scan_reports_an_empty_feasible_subspace(entry):
    from tunempc_amd import closed_loop as cl
    c = lh.case_no_feasible_subspace()
    f = to_dev if entry == 'device' else (lambda x: x)
    r = cl.horizon_closed_loop_batch(f(c['A']), f(c['B']), f(c['Hc']), (1, 4), terminal='cost', J=f(c['J']))
    ref = cr.receding_horizon(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], 1, 'cost', None)
    print('   rho %s  status %s  subres %s' % (r['rho'], r['status'], r['subres']))
    assert r['status'].tolist() == [[0, 5]] and np.isnan(r['rho'][0, 1]) and np.isnan(r['subres'][0, 1]) and np.isnan(to_host(dict(P=r['Phi']))['P'][0, 1]).all()
    assert abs(r['rho'][0, 0] - ref['rho']) <= PARITY * max(1.0, ref['rho'])
    # N = 1 is served, but its law does not look one stage ahead: the state leaves the feasible set of the next phase (and rho = 10.9 > 1), which subres shows
    assert abs(r['subres'][0, 0] - ref['subres']) <= PARITY * max(1.0, ref['subres']) and ref['subres'] > 1.0


# ----------------------------------------------------------------------------- 6. the trajectory-level certificate
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', cr.CASES, ids=[c.__name__ for c in cr.CASES])
def test_telescoping_identity_on_the_reference_cases(entry, case):
    """Random K, T = 2p + 1, phase0 = p - 1, as the numpy reference does it in test_closed_loop_cpu.py; H and Hc are equivalent by construction."""
    from tunempc_amd import closed_loop as cl
    d = as_batch(cr.with_feedback(case))
    p = d['A'].shape[1]
    f = to_dev if entry == 'device' else (lambda x: x)
    r = cl.cost_equivalence_batch(f(d['A']), f(d['B']), f(d['H']), f(d['Hc']), f(d['P']), f(d['K']), f(d['X0']), 2 * p + 1, p - 1)
    print('   %s %s: defect %s  defect_rel %s' % (case.__name__, entry, r['defect'], r['defect_rel']))
    assert all(isinstance(v, np.ndarray) for v in r.values()) and not r['status'].any() and not r['rowres'].any()
    assert r['defect_rel'].max() <= 10.0 * TELESCOPING_DEFECT_REL
    ref = cr.rollout(d['A'][0], d['B'][0], d['K'][0], d['X0'][0], 2 * p + 1, p - 1, H=d['H'][0], Hc=d['Hc'][0])
    assert relmax(r['L'][0], ref['L']) <= PARITY and relmax(r['Lc'][0], ref['Lc']) <= PARITY


@pytest.mark.parametrize('entry', ENTRIES)
def test_certificate_after_a_real_solve(entry):
    """convexify_batch on a small synthetic batch (p 3, nx 3, nu 2, 4 problems), then the rollout of the periodic gains of the Hc side with both costs:
    defect_rel is at or below the larger of ten times the figure of the numpy reference and the relative accuracy at which the solver returned dHc against
    its own P (max|dHc - calH(P)| / max|dHc|, measured here from the outputs of the solve, not from the rollout)."""
    from tunempc_amd import closed_loop as cl, convexifier, lqr
    from tunempc_amd.synthetic import gen_batch
    A, B, H = gen_batch(21, 4, 3, 3, 2)
    res = convexifier.convexify_batch(A, B, H)
    assert (res['status'] == 0).all()
    E = np.concatenate([A, B], axis=3)
    calH = np.einsum('bkji,bkjl,bklm->bkim', E, np.roll(res['P'], -1, axis=1), E)
    calH[:, :, :3, :3] -= res['P']
    floor = np.abs(res['dHc'] - calH).max() / np.abs(res['dHc']).max()
    Hc = np.ascontiguousarray(H + res['dHc'])
    K = lqr.periodic_lqr_batch(A, B, Hc)
    assert not K['status'].any()
    X0 = np.random.default_rng(22).standard_normal((4, 4, 3))
    f = to_dev if entry == 'device' else (lambda x: x)
    r = cl.cost_equivalence_batch(f(A), f(B), f(H), f(Hc), f(np.ascontiguousarray(res['P'])), f(K['K']), f(X0), 7)
    bound = max(10.0 * TELESCOPING_DEFECT_REL, floor)
    print('   defect_rel %s  floors: reference x 10 = %.1e, solver %.2e  rho %s' % (r['defect_rel'], 10.0 * TELESCOPING_DEFECT_REL, floor, K['rho']))
    assert not r['status'].any() and r['defect_rel'].shape == (4, 4) and r['defect_rel'].max() <= bound
    # the contrast: with the P of another problem the identity fails, so the certificate can fail
    wrong = cl.cost_equivalence_batch(f(A), f(B), f(H), f(Hc), f(np.ascontiguousarray(np.roll(res['P'], 1, axis=0))), f(K['K']), f(X0), 7)
    assert wrong['defect_rel'].min() > 1e-4


# ----------------------------------------------------------------------------- 7. non-finite
@pytest.mark.parametrize('entry', ENTRIES)
def test_an_overflowing_member_ends_with_status_3_and_leaves_the_other_alone(entry):
    """A = 1e200 I, K = 0: x_1 = 1e200 x_0 is finite, l_1 and x_2 overflow to inf in ordinary arithmetic -> the states of that member stop at step 1."""
    d, _, _ = small('wrap')
    d = {k: (None if v is None else v.copy()) for k, v in d.items()}
    d['A'][1] = 1e200 * np.eye(3); d['K'][1] = 0.0
    out = run(entry, d, 4, 0)
    assert (out['status'][1] == 3).all() and (out['steps'][1] == 1).all() and (out['status'][0] == 0).all() and (out['steps'][0] == 4).all()
    assert np.isfinite(out['X'][1, :, :2]).all() and np.isnan(out['X'][1, :, 2:]).all() and np.isnan(out['XT'][1]).all()
    assert np.isfinite(out['U'][1, :, :1]).all() and np.isnan(out['U'][1, :, 1:]).all()
    for k in STEP_KEYS:
        assert np.isfinite(out[k][1, :, :1]).all() and np.isnan(out[k][1, :, 1:]).all(), k
    assert np.isnan(out['L'][1]).all() and np.isnan(out['Lc'][1]).all() and np.isfinite(out['xmax'][1]).all()
    alone = run(entry, d, 4, 0, members=[0])
    for k in ALL_KEYS:
        np.testing.assert_array_equal(out[k][0], alone[k][0], err_msg=k)


@pytest.mark.parametrize('entry', ENTRIES)
def test_a_non_finite_input_is_status_3_for_the_states_that_meet_it(entry):
    """A NaN in H of stage 1 of member 0 (met at step 1 from phase 0), an inf in one initial state of member 1 (step 0; its tile neighbours go on)."""
    d, _, _ = small('wrap')
    d = {k: (None if v is None else v.copy()) for k, v in d.items()}
    d['H'][0, 1, 4, 4] = np.nan; d['X0'][1, 2, 0] = np.inf
    out = run(entry, d, 5, 0)
    assert (out['status'][0] == 3).all() and (out['steps'][0] == 1).all()
    assert out['status'][1].tolist() == [0, 0, 3, 0, 0] and out['steps'][1].tolist() == [5, 5, 0, 5, 5]
    assert np.isnan(out['U'][1, 2]).all() and np.isnan(out['X'][1, 2, 1:]).all() and np.isnan(out['xmax'][1, 2])
    clean, _, _ = small('wrap')
    ok = run(entry, clean, 5, 0)
    for k in ALL_KEYS:
        np.testing.assert_array_equal(out[k][1, [0, 1, 3, 4]], ok[k][1, [0, 1, 3, 4]], err_msg=k)


# ----------------------------------------------------------------------------- 8. the reference's calling style
def test_closed_loop_sim_on_the_c1_golden():
    """p = 1, the gains of periodic_lqr in the loop for 200 steps: the log of the reference, and the Riccati telescoping sum
    sum_t l_t = 1/2 x_0' Pi x_0 - 1/2 x_T' Pi x_T."""
    from tunempc_amd import closed_loop as cl, lqr
    g = np.load(os.path.join(GOLDEN, 'c1_convex_lqr.npz'))
    A, B, H, Hc = (np.ascontiguousarray(g[k][0, 0], dtype=np.float64) for k in ('A', 'B', 'H', 'Hc'))
    nx = A.shape[0]
    Q, R, N = H[:nx, :nx], H[nx:, nx:], H[:nx, nx:]
    K, Pi, rho = lqr.periodic_lqr(A, B, Q, R, N)
    x0 = np.random.default_rng(1).standard_normal(nx)
    log = cl.closed_loop_sim(A, B, K, x0, 200, Q=Q, R=R, N=N, dHc=[Hc - H])
    assert sorted(log) == ['h', 'l', 'lc', 'u', 'x'] and len(log['x']) == 201 and len(log['u']) == len(log['l']) == len(log['h']) == len(log['lc']) == 200
    assert log['x'][0].shape == (nx,) and log['u'][0].shape == (B.shape[1],) and log['h'][0].shape == (0,)
    np.testing.assert_array_equal(log['x'][0], x0)
    want = 0.5 * x0 @ Pi[0] @ x0 - 0.5 * log['x'][-1] @ Pi[0] @ log['x'][-1]
    print('   rho %.6f  sum l %.15e  telescoped %.15e' % (rho, sum(log['l']), want))
    assert abs(sum(log['l']) - want) <= PARITY * abs(want)
    plain = cl.closed_loop_sim(A, B, K[0], x0, 3)
    assert sorted(plain) == ['h', 'l', 'u', 'x'] and plain['l'] == [0.0] * 3
    np.testing.assert_array_equal(np.stack(plain['x']), np.stack(log['x'][:4]))


def test_cost_equivalence_in_the_calling_style_of_convexify():
    from tunempc_amd import closed_loop as cl
    d = cr.with_feedback(lh.case_ragged_rows)
    p, nx = 3, 3
    lst = lambda f: [f(k) for k in range(p)]
    H = d['H']
    args = (lst(lambda k: d['A'][k]), lst(lambda k: d['B'][k]), lst(lambda k: H[k][:nx, :nx]), lst(lambda k: H[k][nx:, nx:]), lst(lambda k: H[k][:nx, nx:]))
    r = cl.cost_equivalence(*args, lst(lambda k: d['Hc'][k] - H[k]), lst(lambda k: d['P'][k]), lst(lambda k: d['K'][k]), d['X0'], 7, 2)
    b = cl.cost_equivalence_batch(d['A'][None], d['B'][None], H[None], d['Hc'][None], d['P'][None], d['K'][None], d['X0'][None], 7, 2)
    assert r['defect_rel'].shape == (4,) and r['defect_rel'].max() <= 100.0 * TELESCOPING_DEFECT_REL      # (Hc - H + H is not Hc to the last bit)
    np.testing.assert_array_equal(r['status'], b['status'][0])
    assert relmax(r['L'], b['L'][0]) <= PARITY


# ----------------------------------------------------------------------------- 9. refusals on device tensors
def test_shapes_beyond_the_layout_are_refused_before_a_launch():
    from tunempc_amd import closed_loop as cl
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64'):
        cl.closed_loop_batch(z(1, 2, 40, 40), z(1, 2, 40, 30), z(1, 2, 30, 40), z(1, 1, 40), 3)
    with pytest.raises(ValueError, match='phase0 must be an int in 0 .. p - 1 = 1'):
        cl.closed_loop_batch(z(1, 2, 3, 3), z(1, 2, 3, 1), z(1, 2, 1, 3), z(1, 1, 3), 3, phase0=2)
