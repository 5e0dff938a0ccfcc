"""GPU tests of the warm-started MPC step and loop (csrc/tmpc_mpc_qp.h, the WARM instantiations; tunempc_amd.mpc_qp: guess=, guess_shift=, warm=,
warm_floor=, mpc_closed_loop_plant) against the numpy warm loop of tests/mpc_qp_warm_reference.py and against the cold calls of the same batch.

Bounds.  Against the numpy warm loop: 10 x the family's (a)-against-(b) bound, what the family's own GPU tests use against its reference (both loops run on
iterates that lie within that bound of the same truth).  The warm loop against the cold loop: twice that, both being solutions at `tol`; a single step from a guess (the alpha sweep) against its cold call: that
bound itself.  The plant callback with a linear
plant against the loop in one launch: 1e-12.  Bit-identity where the kernel promises it: host against device, an instance alone against the same instance
among more than 512 others, the other instances of a batch beside a NaN guess.  Iteration counts against numpy are printed, not compared (the rule of the
families' GPU tests); warm against cold they are compared: the total over the steps >= 1 is strictly lower per case."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_warm_reference as wr  # noqa: E402

STEPS = wr.STEPS
NAMES = ['box_nu1', 'mixed_small', 'single_phase', 'soft', 'eq', 'affine', 'quad_l12', 'quad_pure', 'box_bench']
GUESS = ('X', 'U', 'lam', 'eps', 'nu', 'nu_term')


def relmax(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if b.size else 0.0


def to_dev(x):
    return x if x is None or isinstance(x, str) else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def to_host(out):
    return {k: (np.ascontiguousarray(v.cpu().numpy()) if isinstance(v, torch.Tensor) else (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v))
            for k, v in out.items()}


def arguments(entry, pr, steps=None, X0=None, members=slice(None), states=slice(None)):
    """(args, kwargs) of mpc_qp_batch (steps None) or mpc_closed_loop_batch for (a slice of) a problem of mpc_qp_warm_reference."""
    f = to_dev if entry == 'device' else (lambda x: x)
    pick = lambda x: x if isinstance(x, str) else f(np.ascontiguousarray(x[members]))
    X0 = np.ascontiguousarray((pr['X0'] if X0 is None else X0)[members][:, states])
    kw = {k: pick(v) for k, v in pr['opt'].items()}
    if steps is not None and 'disturbance' in pr['loop']:
        kw['disturbance'] = f(np.ascontiguousarray(pr['loop']['disturbance'][members][:, states, :steps]))
    return (pick(pr['A']), pick(pr['B']), pick(pr['H']), f(X0), pr['N']), kw


def run(entry, pr, steps=None, guess=None, **kw):
    from tunempc_amd import mpc_qp as m
    sel = {k: kw.pop(k) for k in ('X0', 'members', 'states') if k in kw}
    args, opt = arguments(entry, pr, steps, **sel)
    if guess is not None:
        kw['guess'] = {k: (to_dev(v) if entry == 'device' else v) for k, v in guess.items()}
    out = m.mpc_qp_batch(*args, pr['k0'], **opt, **kw) if steps is None else m.mpc_closed_loop_batch(*args, steps, pr['k0'], **opt, **kw)
    return to_host(out)


def assert_same(a, b, keys=None):
    for k in (keys or a.keys()):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def guess_of(out):
    return {k: out[k] for k in GUESS if out.get(k) is not None}


@functools.lru_cache(maxsize=None)
def loops(name, entry):
    """The cold and the warm loop of a problem through one entry, once per process."""
    pr = wr.problems()[name]
    return run(entry, pr, STEPS), run(entry, pr, STEPS, warm=True)


# ----------------------------------------------------------------------------- 1. the warm loop against the numpy warm loop and against the cold loop
@pytest.mark.parametrize('name', NAMES)
def test_warm_loop_against_the_numpy_warm_loop_and_the_cold_loop(name):
    pr = wr.problems()[name]
    parity = 10 * pr['bound']
    ref = wr.loops(name, True)
    cold, warm = loops(name, 'device')
    nb, ns = pr['X0'].shape[:2]
    assert 'warm' not in cold and warm['warm'].shape == (nb, ns, STEPS) and warm['warm'].dtype == np.int32
    assert not cold['status'].any() and not warm['status'].any() and (warm['steps'] == STEPS).all()
    np.testing.assert_array_equal(warm['iters_total'], warm['iters'].sum(axis=2))
    for b in range(nb):
        for s in range(ns):
            r = ref[b][s]
            assert r['status'] == 0
            e = dict(X=relmax(warm['X'][b, s], r['X']), U=relmax(warm['U'][b, s], r['U']))
            c = dict(X=relmax(warm['X'][b, s], cold['X'][b, s]), U=relmax(warm['U'][b, s], cold['U'][b, s]))
            print('   %s %d.%d: warm iters %s (numpy %s) cold %s | vs numpy %s | vs cold %s' % (name, b, s, warm['iters'][b, s].tolist(), r['iters'].tolist(),
                                                                                           cold['iters'][b, s].tolist(), {q: '%.1e' % v for q, v in e.items()},
                                                                                           {q: '%.1e' % v for q, v in c.items()}))
            assert max(e.values()) <= parity, e
            assert max(c.values()) <= 2 * parity, c
            np.testing.assert_array_equal(warm['warm'][b, s], r['warm'])
    assert (warm['warm'][:, :, 0] == 0).all() and np.isin(warm['warm'][:, :, 1:], (1, 2)).all()
    np.testing.assert_array_equal(warm['nact'], cold['nact'])
    tw, tc = int(warm['iters'][:, :, 1:].sum()), int(cold['iters'][:, :, 1:].sum())
    print('   %s: iterations over the steps >= 1: warm %d, cold %d' % (name, tw, tc))
    assert tw < tc


# ----------------------------------------------------------------------------- 2. the plant callback
def linear_plant(pr, entry):
    A, B, p, k0 = pr['A'], pr['B'], pr['A'].shape[1], pr['k0']
    W = pr['loop'].get('disturbance')
    if entry == 'device':
        A, B, W = to_dev(A), to_dev(B), to_dev(W)

    def plant(t, X, U):
        k = (k0 + t) % p
        Xn = (A[:, k][:, None] @ X[..., None])[..., 0] + (B[:, k][:, None] @ U[..., None])[..., 0]
        return Xn if W is None else Xn + W[:, :, t]
    return plant


@pytest.mark.parametrize('entry', ['host', 'device'])
@pytest.mark.parametrize('name', ['box_nu1', 'eq', 'affine', 'quad_l12'])
def test_plant_callback_with_a_linear_plant_is_the_warm_loop(name, entry):
    from tunempc_amd import mpc_qp as m
    pr = wr.problems()[name]
    _, warm = loops(name, entry)
    args, opt = arguments(entry, pr)
    out = to_host(m.mpc_closed_loop_plant(*args, STEPS, linear_plant(pr, entry), pr['k0'], **opt))
    assert sorted(out) == sorted(warm), (sorted(out), sorted(warm))
    e = {k: relmax(out[k], warm[k]) for k in ('X', 'U', 'XT', 'u0', 'hres')}
    bits = all(np.array_equal(out[k], warm[k]) for k in ('X', 'U'))
    print('   %s %s: plant callback against the loop in one launch %s, bit-equal %s' % (name, entry, {q: '%.1e' % v for q, v in e.items()}, bits))
    assert max(e.values()) <= 1e-12, e
    for k in ('iters', 'warm', 'nact', 'status', 'steps', 'iters_total', 'iters_max'):
        np.testing.assert_array_equal(out[k], warm[k], err_msg=k)
    assert out['info'].shape == warm['info'].shape
    np.testing.assert_array_equal(out['info'][..., :4], warm['info'][..., :4])


@pytest.mark.parametrize('entry', ['host', 'device'])
def test_plant_callback_with_a_cubic_plant(entry):
    from tunempc_amd import mpc_qp as m
    pr = wr.problems()['box_nu1']
    lin = linear_plant(pr, entry)
    plant = lambda t, X, U: lin(t, X, U) + 0.05 * X ** 3
    args, opt = arguments(entry, pr)
    raw = m.mpc_closed_loop_plant(*args, STEPS, plant, pr['k0'], **opt)
    for t in range(STEPS):
        want = plant(t, raw['X'][:, :, t], raw['U'][:, :, t])
        assert bool((raw['X'][:, :, t + 1] == want).all()), t
    out = to_host(raw)
    cold = to_host(m.mpc_closed_loop_plant(*args, STEPS, plant, pr['k0'], warm=False, **opt))
    print('   cubic %s: iters warm %s cold %s' % (entry, out['iters'][0].tolist(), cold['iters'][0].tolist()))
    assert not out['status'].any() and (out['steps'] == STEPS).all() and np.isfinite(out['X']).all()
    assert (out['warm'][:, :, 0] == 0).all() and np.isin(out['warm'][:, :, 1:], (1, 2)).all() and not cold['warm'].any()
    assert relmax(out['X'], cold['X']) <= 20 * pr['bound'] and relmax(out['U'], cold['U']) <= 20 * pr['bound']
    assert np.abs(out['X'] - loops('box_nu1', entry)[1]['X']).max() > 1e-6    # (the cubic term is felt)


# ----------------------------------------------------------------------------- 3. a guess for the same phase: the sweep along a line of initial states
@pytest.mark.parametrize('name', ['box_nu1', 'soft', 'eq', 'quad_pure', 'box_bench'])
def test_alpha_sweep_with_the_previous_solution_as_the_guess(name):
    pr = wr.problems()[name]
    parity = 10 * pr['bound']
    prev = None
    for alpha in (0.6, 0.7, 0.8, 0.9, 1.0):                                 # (towards the case's own X0: every state on the line is feasible)
        X0 = alpha * pr['X0']
        cold = run('device', pr, X0=X0)
        assert not cold['status'].any()
        if prev is not None:
            out = run('device', pr, X0=X0, guess=guess_of(prev))
            e = {k: relmax(out[k], cold[k]) for k in ('u0', 'X', 'U')}
            ls = max(1.0, np.abs(cold['lam']).max())
            e['lam'] = np.abs(out['lam'] - cold['lam']).max() / ls
            print('   %s alpha %.1f: iters %s (cold %s) warm %s | %s' % (name, alpha, out['iters_total'].reshape(-1).tolist(), cold['iters_total'].reshape(-1).tolist(),
                                                                   out['warm'].reshape(-1).tolist(), {q: '%.1e' % v for q, v in e.items()}))
            assert not out['status'].any() and np.isin(out['warm'], (1, 2)).all() and out['warm'].shape == cold['status'].shape
            assert max(e.values()) <= parity, e
            np.testing.assert_array_equal(out['nact'], cold['nact'])
            np.testing.assert_array_equal(out['X'][:, :, 0], X0)
            prev = out
        else:
            prev = cold


# ----------------------------------------------------------------------------- 4. a NaN guess in one instance
@pytest.mark.parametrize('name', ['box_nu1', 'soft'])
def test_a_nan_guess_starts_that_instance_cold_and_leaves_the_others_alone(name):
    pr = wr.problems()[name]
    cold = run('device', pr)
    g = guess_of(cold)
    clean = run('device', pr, guess=g, guess_shift=0)
    nb, ns = pr['X0'].shape[:2]
    b0, s0 = nb - 1, ns - 1
    for key in ('X', 'lam'):
        bad = {k: v.copy() for k, v in g.items()}
        bad[key][b0, s0].reshape(-1)[-1] = np.nan
        out = run('device', pr, guess=bad)
        assert out['warm'][b0, s0] == 0 and not out['status'].any()
        others = np.ones((nb, ns), bool); others[b0, s0] = False
        assert (out['warm'][others] == 1).all() or nb * ns == 1
        for k in ('u0', 'X', 'U', 'lam', 'x1', 'info', 'warm'):
            np.testing.assert_array_equal(out[k][others], clean[k][others], err_msg=k)
        assert out['iters_total'][b0, s0] == cold['iters_total'][b0, s0]
        bits = all(np.array_equal(out[k][b0, s0], cold[k][b0, s0]) for k in ('u0', 'X', 'U', 'lam'))
        print('   %s NaN in %s: the cold start of the WARM kernel against the cold kernel: bit-equal %s' % (name, key, bits))
        for k in ('u0', 'X', 'U'):
            assert relmax(out[k][b0, s0], cold[k][b0, s0]) <= 1e-12, k


# ----------------------------------------------------------------------------- 5. host against device
@pytest.mark.parametrize('name', ['box_nu1', 'mixed_small', 'soft', 'eq', 'affine', 'quad_l12', 'quad_pure'])
def test_host_and_device_agree_bit_for_bit(name):
    pr = wr.problems()[name]
    (_, hw), (_, dw) = loops(name, 'host'), loops(name, 'device')
    assert_same(hw, dw)
    cold = run('host', pr)
    h, d = (run(e, pr, X0=0.9 * pr['X0'], guess=guess_of(cold), warm_floor=3e-3) for e in ('host', 'device'))
    assert not h['status'].any() and np.isin(h['warm'], (1, 2)).all()
    assert_same(h, d)
    hs, ds = (run(e, pr, STEPS, guess=guess_of(cold), guess_shift=1, warm=True) for e in ('host', 'device'))
    assert_same(hs, ds)
    assert np.isin(hs['warm'][:, :, 0], (1, 2)).all()


# ----------------------------------------------------------------------------- 6. an instance does not depend on ns, the slot or the other instances
def test_an_instance_does_not_depend_on_the_slot_or_on_the_others():
    pr = wr.problems()['single_phase']
    rng = np.random.default_rng(91)
    nx = pr['X0'].shape[2]
    X0 = np.concatenate([pr['X0'][:1], 0.8 * rng.standard_normal((1, 597, nx))], axis=1)       # 600 instances: slots are reused after a warm step
    out = run('device', pr, STEPS, X0=X0, members=slice(0, 1), warm=True)
    cold = run('device', pr, STEPS, X0=X0, members=slice(0, 1))
    assert not out['status'].any() and not cold['status'].any()              # (an input box: every state is feasible)
    assert int(out['iters'][:, :, 1:].sum()) < int(cold['iters'][:, :, 1:].sum())
    for s in (0, 2, 300, 511, 512, 599):
        one = run('device', pr, STEPS, X0=X0, members=slice(0, 1), states=slice(s, s + 1), warm=True)
        for k in ('X', 'U', 'iters', 'nact', 'hres', 'XT', 'u0', 'info', 'warm'):
            np.testing.assert_array_equal(one[k][:, 0], out[k][:, s], err_msg='%s of state %d' % (k, s))
    _, small = loops('single_phase', 'device')
    for k in ('X', 'U', 'iters', 'warm', 'info'):
        np.testing.assert_array_equal(small[k][0, :3], out[k][0, :3], err_msg=k)


# ----------------------------------------------------------------------------- 7. the retry: a bad but finite guess that exhausts a small max_iter
def test_a_bad_guess_that_exhausts_max_iter_is_retried_cold():
    from test_mpc_qp_warm_cpu import bad_guess_case
    pr, guess, max_iter, b_ref = bad_guess_case()
    cold = run('device', pr, max_iter=max_iter)
    out = run('device', pr, guess=guess, max_iter=max_iter)
    print('   retry: warm codes %s iters %s (cold %s), numpy codes %s' % (out['warm'].reshape(-1).tolist(), out['iters_total'].reshape(-1).tolist(),
                                                                    cold['iters_total'].reshape(-1).tolist(), [r['warm'] for r in b_ref]))
    assert not cold['status'].any() and not out['status'].any()
    np.testing.assert_array_equal(out['warm'].reshape(-1), [r['warm'] for r in b_ref])
    assert (out['warm'] == 2).any()
    two = out['warm'] == 2
    np.testing.assert_array_equal(out['iters_total'][two], max_iter + cold['iters_total'][two])
    for k in ('u0', 'X', 'U', 'lam'):
        assert relmax(out[k][two], cold[k][two]) <= 1e-12, k
