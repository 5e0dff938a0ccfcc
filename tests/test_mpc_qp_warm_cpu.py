"""CPU tests of the warm start of the constrained MPC step: the rule on the numpy reference (tests/mpc_qp_warm_reference.py), the Python layer (keywords,
validation before the library is loaded, routing, pinned signatures) and the C entries' argument checks.  No device is needed.

The warm loop is held to the polished truth (method (b)) of each family's own reference at every step, with that family's certificate and its bound for
(a) against (b): the warm iterate is one more iterate that met the same stop test."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mpc_qp_warm_reference as wr

NAMES = ['box_nu1', 'mixed_small', 'single_phase', 'soft', 'eq', 'affine', 'quad_l12', 'quad_pure', 'box_bench']
MARGIN_MIN = 1e-4            # the smallest margin the families' CPU tests accept (mpc_qp_soft_reference.MARGIN_MIN; the hard cases ask 1e-3 of their own X0)


# ----------------------------------------------------------------------------- 1. the rule on the reference
@pytest.mark.parametrize('name', NAMES)
def test_warm_loop_reaches_the_polished_truth_at_every_step_in_fewer_iterations(name):
    pr = wr.problems()[name]
    cold, warm = wr.loops(name, False), wr.loops(name, True)
    tc = tw = 0
    worst = {}
    for b, (cb, wb) in enumerate(zip(cold, warm)):
        kw = wr.member_kw(pr, b)
        for s, (c, w) in enumerate(zip(cb, wb)):
            assert c['status'] == 0 and w['status'] == 0 and w['steps'] == wr.STEPS
            assert w['warm'][0] == wr.COLD and (w['warm'][1:] == wr.WARM).all() and not c['warm'].any()
            W = pr['loop'].get('disturbance')
            for t, r in enumerate(w['sols']):
                fam, tr = wr.truth(pr['A'][b], pr['B'][b], pr['H'][b], pr['N'], (pr['k0'] + t) % pr['A'].shape[1], w['X'][t], **kw)
                assert fam == pr['fam'] and tr['b']['certificate'] and tr['b']['margin'] >= MARGIN_MIN, (t, tr['b']['margin'])
                e = wr.against_truth(fam, tr, r)
                for k, v in e.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                assert max(e.values()) <= pr['bound'], (b, s, t, e)
            tc += int(c['iters'][1:].sum()); tw += int(w['iters'][1:].sum())
            print('   %s %d.%d: cold %s warm %s' % (name, b, s, c['iters'].tolist(), w['iters'].tolist()))
            assert W is None or W.shape[2] >= wr.STEPS
    print('   %s: steps >= 1: cold %d warm %d; warm iterates against the polished truth %s (bound %.0e)' % (name, tc, tw, {k: '%.1e' % v for k, v in worst.items()}, pr['bound']))
    assert tw < tc


@pytest.mark.parametrize('name', NAMES)
def test_the_floors_hold_at_every_warm_start(name):
    import mpc_qp_quad_reference as mqq
    fl = wr.WARM_FLOOR
    seen = 0
    for wb in wr.loops(name, True):
        for w in wb:
            for r in w['sols'][1:]:
                st, cvec, zvec = r['start'], r['cvec'], r['zvec']
                assert st is not None
                hard, two, pure, quad = mqq.kinds(cvec, zvec)
                tot = np.where(two, np.where(two, cvec, 0.0) + np.where(quad, zvec, 0.0) * st['e'], 0.0)
                assert (tot[two] - st['lam'][two] - st['nu'][two] == 0.0).all()                      # exactly
                small = two & (tot < 2 * fl)
                assert (st['lam'][small] == 0.5 * tot[small]).all() and (st['nu'][small] == st['lam'][small]).all()
                big = two & ~small
                assert (st['s'] >= fl).all() and (st['lam'][~two] >= fl).all() and (st['lam'][big] >= fl).all() and (st['nu'][big] >= fl * (1 - 1e-15)).all()
                assert (st['e'][two] >= fl).all() and (st['e'][~two] == 0).all()
                seen += 1
    assert seen


def test_the_shift_is_the_stated_one():
    pr = wr.problems()['mixed_small']
    b, s = 0, 1
    kw = wr.member_kw(pr, b)
    A, B, N, p = pr['A'][b], pr['B'][b], pr['N'], pr['A'].shape[1]
    r = wr.solve_warm(A, B, pr['H'][b], N, pr['k0'], pr['X0'][b, s], **kw)
    g = {k: r[k] for k in ('X', 'U', 'Lam', 'Eps', 'Nu', 'NuT')}
    x0 = A[pr['k0']] @ r['X'][0] + B[pr['k0']] @ r['U'][0] + 0.01
    k1 = (pr['k0'] + 1) % p
    sh = wr.shift_guess(g, x0, A, B, k1, shift=1)
    np.testing.assert_array_equal(sh['X'][0], x0)
    np.testing.assert_array_equal(sh['X'][1:N], r['X'][2:]); np.testing.assert_array_equal(sh['U'][:N - 1], r['U'][1:]); np.testing.assert_array_equal(sh['U'][N - 1], r['U'][N - 1])
    kl = (k1 + N - 1) % p
    np.testing.assert_array_equal(sh['X'][N], A[kl] @ sh['X'][N - 1] + B[kl] @ sh['U'][N - 1])
    np.testing.assert_array_equal(sh['Lam'][:N - 1], r['Lam'][1:]); assert not sh['Lam'][N - 1].any()
    same = wr.shift_guess(g, x0, A, B, pr['k0'], shift=0)
    np.testing.assert_array_equal(same['X'][1:], r['X'][1:]); np.testing.assert_array_equal(same['U'], r['U']); np.testing.assert_array_equal(same['X'][0], x0)


@pytest.mark.parametrize('name', ['box_nu1', 'soft', 'eq', 'quad_pure'])
def test_a_nan_guess_gives_the_cold_iterate_and_the_cold_count(name):
    pr = wr.problems()[name]
    kw = wr.member_kw(pr, 0)
    args = (pr['A'][0], pr['B'][0], pr['H'][0], pr['N'], pr['k0'], pr['X0'][0, 0])
    cold = wr.solve_warm(*args, **kw)
    g = {k: cold[k].copy() for k in ('X', 'U', 'Lam', 'Eps', 'Nu', 'NuT')}
    g['U'][-1, -1] = np.nan
    r = wr.solve_warm(*args, g, 0, **kw)
    assert r['warm'] == wr.COLD and r['start'] is None and r['iters'] == cold['iters'] and r['status'] == 0
    for k in ('v', 'lam', 's', 'e', 'nu', 'nue'):
        np.testing.assert_array_equal(r['a'][k], cold['a'][k])
    fam, tr = wr.truth(*args, **kw)                                          # the restated loop started cold is the family's own (a): same count
    assert cold['iters'] == tr['a']['iters'] and np.abs(cold['a']['v'] - tr['a']['v']).max() <= 1e-12


def bad_guess_case():
    """box_nu1 with max_iter = 10 and, as the guess of instance s, the solution of instance s + 3 (mod 4): on the reference the warm attempts of two instances
    run out of iterations (13 and 11 would be needed) and are solved again cold (7 iterations), the other two converge warm in 8 -> (problem, the guess in the
    keys of mpc_qp_batch, max_iter, the dicts of solve_warm in instance order)."""
    pr = wr.problems()['box_nu1']
    nb, ns = pr['X0'].shape[:2]
    assert nb == 1
    kw = wr.member_kw(pr, 0)
    args = lambda s: (pr['A'][0], pr['B'][0], pr['H'][0], pr['N'], pr['k0'], pr['X0'][0, s])
    sols = [wr.solve_warm(*args(s), **kw) for s in range(ns)]
    other = [sols[(s + 3) % ns] for s in range(ns)]
    guess = {lo: np.stack([o[up] for o in other])[None] for lo, up in (('X', 'X'), ('U', 'U'), ('lam', 'Lam'))}
    max_iter = 10
    ref = [wr.solve_warm(*args(s), {k: other[s][k] for k in ('X', 'U', 'Lam', 'Eps', 'Nu', 'NuT')}, 0, max_iter=max_iter, **kw) for s in range(ns)]
    return pr, guess, max_iter, ref


def test_a_bad_but_finite_guess_that_exhausts_max_iter_is_retried_cold():
    pr, guess, max_iter, ref = bad_guess_case()
    kw = wr.member_kw(pr, 0)
    codes = [r['warm'] for r in ref]
    print('   codes %s iters %s' % (codes, [r['iters'] for r in ref]))
    assert codes.count(wr.RETRIED) >= 1 and codes.count(wr.WARM) >= 1
    for s, r in enumerate(ref):
        cold = wr.solve_warm(pr['A'][0], pr['B'][0], pr['H'][0], pr['N'], pr['k0'], pr['X0'][0, s], max_iter=max_iter, **kw)
        assert cold['status'] == 0 and r['status'] == 0
        if r['warm'] == wr.RETRIED:
            assert r['iters'] == max_iter + cold['iters'] and r['start'] is not None
            for k in ('v', 'lam', 's'):
                np.testing.assert_array_equal(r['a'][k], cold['a'][k])
        else:
            assert r['iters'] <= max_iter and np.abs(r['a']['v'] - cold['a']['v']).max() <= 1e-9


# ----------------------------------------------------------------------------- 2. the Python layer
class _Routed(Exception):
    pass


@pytest.fixture
def recorders(monkeypatch):
    """The twelve binding functions of _lib replaced by recorders, load_library by a tripwire."""
    from tunempc_amd import _lib
    for lv in ('', 'soft_', 'eq_', 'aff_', 'quad_', 'warm_'):
        for e in ('host', 'device'):
            nm = 'mpc_qp_%sbatch_%s' % (lv, e)

            def rec(*a, _nm=nm, **k):
                raise _Routed(_nm, a)
            monkeypatch.setattr(_lib, nm, rec)
    monkeypatch.setattr(_lib, 'load_library', lambda: (_ for _ in ()).throw(AssertionError('the library was loaded')))


def small():
    z = np.zeros
    return (z((1, 2, 3, 3)), z((1, 2, 3, 1)), z((1, 2, 4, 4)), z((1, 2, 3))), dict(D=z((1, 2, 2, 4)), d=z((1, 2, 2)))


def guess_for(N=3, nd=2, **extra):
    z = np.zeros
    g = dict(X=z((1, 2, N + 1, 3)), U=z((1, 2, N, 1)), lam=z((1, 2, N, nd)))
    g.update(extra)
    return g


def test_calls_are_routed_to_the_warm_entry_only_with_the_new_keywords(recorders):
    from tunempc_amd import mpc_qp as m
    (A, B, H, X0), rows = small()
    pen = np.ones((1, 2, 2))
    old = [(dict(), 'mpc_qp_batch_host'), (rows, 'mpc_qp_batch_host'), (dict(rows, penalty=pen), 'mpc_qp_soft_batch_host'),
           (dict(terminal='constraint'), 'mpc_qp_eq_batch_host'), (dict(rows, offset=np.zeros((1, 2, 3))), 'mpc_qp_aff_batch_host'),
           (dict(rows, penalty2=pen), 'mpc_qp_quad_batch_host')]
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        for kw, name in old:
            with pytest.raises(_Routed) as ei:
                f(A, B, H, X0, 3, *extra, **kw)
            assert ei.value.args[0] == name
    z = np.zeros
    new = [(m.mpc_qp_batch, (), dict(rows, guess=guess_for()), (2, 1e-2)), (m.mpc_qp_batch, (), dict(rows, guess=guess_for(), guess_shift=1, warm_floor=1e-3), (6, 1e-3)),
           (m.mpc_qp_batch, (), dict(guess=dict(X=z((1, 2, 4, 3)), U=z((1, 2, 3, 1)))), (2, 1e-2)),
           (m.mpc_closed_loop_batch, (2,), dict(rows, warm=True), (1, 1e-2)), (m.mpc_closed_loop_batch, (2,), dict(rows, warm=True, guess=guess_for()), (3, 1e-2)),
           (m.mpc_closed_loop_batch, (2,), dict(rows, penalty=pen, warm=True, guess=guess_for(eps=z((1, 2, 3, 2))), guess_shift=1), (7, 1e-2)),
           (m.mpc_closed_loop_batch, (2,), dict(rows, warm_floor=0.5), (0, 0.5)),
           # passed with the default's value: still the warm entry (flags 0: every step cold) and a `warm` key
           (m.mpc_closed_loop_batch, (2,), dict(rows, warm=False), (0, 1e-2)), (m.mpc_closed_loop_batch, (2,), dict(rows, warm_floor=1e-2), (0, 1e-2)),
           (m.mpc_qp_batch, (), dict(rows, guess_shift=0), (0, 1e-2)), (m.mpc_qp_batch, (), dict(rows, guess=None), (0, 1e-2)),
           (m.mpc_qp_batch, (), dict(rows, terminal='constraint', guess=guess_for(nu_term=z((1, 2, 3)))), (2, 1e-2))]
    for f, extra, kw, (flags, floor) in new:
        with pytest.raises(_Routed) as ei:
            f(A, B, H, X0, 3, *extra, **kw)
        name, args = ei.value.args
        assert name == 'mpc_qp_warm_batch_host' and len(args) == 24
        wm = args[15]
        assert wm[0] == flags and wm[1] == floor and len(wm) == 8
        no_guess = kw.get('guess') is None
        assert (wm[2] is None) == no_guess and (wm[4] is None) == (no_guess or 'D' not in kw)
        assert (wm[5] is None) == ('penalty' not in kw or no_guess) and (wm[7] is None) == ('terminal' not in kw)
    one = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)), np.ones(2), 4)
    rows1 = dict(D=np.ones((1, 3)), d=np.ones(1))
    g1 = dict(X=np.zeros((5, 2)), U=np.zeros((4, 1)), lam=np.zeros((4, 1)))
    for call, kw, name in ((m.mpc_step, dict(), 'mpc_qp_batch_host'), (m.mpc_step, dict(guess=g1), 'mpc_qp_warm_batch_host'),
                           (m.mpc_step, dict(guess=g1, guess_shift=1), 'mpc_qp_warm_batch_host'), (m.mpc_step, dict(warm_floor=1e-2), 'mpc_qp_warm_batch_host'),
                           (lambda *a, **k: m.mpc_closed_loop_sim(*a, 3, **k), dict(warm=False), 'mpc_qp_warm_batch_host'),
                           (lambda *a, **k: m.mpc_closed_loop_sim(*a, 3, **k), dict(), 'mpc_qp_batch_host'),
                           (lambda *a, **k: m.mpc_closed_loop_sim(*a, 3, **k), dict(warm=True), 'mpc_qp_warm_batch_host')):
        with pytest.raises(_Routed) as ei:
            call(*one, **rows1, **kw)
        assert ei.value.args[0] == name
    with pytest.raises(_Routed) as ei:                                       # the plant callback: one warm-entry launch per step, the first without a guess
        m.mpc_closed_loop_plant(A, B, H, X0, 3, 2, lambda t, X, U: X, **rows)
    assert ei.value.args[0] == 'mpc_qp_warm_batch_host' and ei.value.args[1][15][0] == 0


def test_validation_errors_are_raised_before_the_library_is_loaded(recorders):
    from tunempc_amd import mpc_qp as m
    (A, B, H, X0), rows = small()
    z = np.zeros
    bad = [(dict(rows, guess=[1]), 'guess must be a dict'), (dict(rows, guess=dict(X=None, U=z((1, 2, 3, 1)), lam=z((1, 2, 3, 2)))), "guess['X']"),
           (dict(rows, guess=guess_for(N=2)), "guess['X'] (1, 2, 4, 3) expected, got (1, 2, 3, 3)"),
           (dict(rows, guess=dict(X=z((1, 2, 4, 3)), U=z((1, 2, 3, 1)))), "guess['lam']"),
           (dict(rows, penalty=np.ones((1, 2, 2)), guess=guess_for()), "guess['eps']"),
           (dict(rows, terminal='constraint', guess=guess_for()), "guess['nu_term']"),
           (dict(rows, J=z((1, 2, 1, 4)), guess=guess_for()), "guess['nu']"),
           (dict(rows, guess=guess_for(), guess_shift=2), 'guess_shift must be 0'), (dict(rows, guess_shift=1), 'guess_shift describes guess'),
           (dict(rows, guess=guess_for(), warm_floor=0.0), 'warm_floor must be'), (dict(rows, warm_floor=float('nan')), 'warm_floor must be'),
           (dict(rows, guess=guess_for(), warm_floor='x'), 'warm_floor must be')]
    for f, extra in ((m.mpc_qp_batch, ()), (m.mpc_closed_loop_batch, (2,))):
        for kw, txt in bad:
            with pytest.raises(ValueError) as ei:
                f(A, B, H, X0, 3, *extra, **kw)
            assert txt in str(ei.value) and f.__name__ in str(ei.value), (txt, str(ei.value))
    with pytest.raises(ValueError, match='warm must be a bool'):
        m.mpc_closed_loop_batch(A, B, H, X0, 3, 2, warm=1, **rows)
    with pytest.raises(TypeError):
        m.mpc_qp_batch(A, B, H, X0, 3, warm=True)                            # (the step has no loop to warm)
    for kw, txt in ((dict(disturbance=z((1, 2, 2, 3))), 'disturbance has no place'), (dict(return_traj=False), 'return_traj has no place')):
        with pytest.raises(ValueError) as ei:
            m.mpc_closed_loop_plant(A, B, H, X0, 3, 2, lambda t, X, U: X, **kw)
        assert txt in str(ei.value)
    with pytest.raises(ValueError, match='plant must be a callable'):
        m.mpc_closed_loop_plant(A, B, H, X0, 3, 2, (A, B))
    with pytest.raises(ValueError, match='steps'):
        m.mpc_closed_loop_plant(A, B, H, X0, 3, 0, lambda t, X, U: X)


SIGNATURES = {
    'mpc_qp_batch': 'A B H X0 horizon phase0 D d ndcnt q Pf tol max_iter return_traj offset qf terminal_rhs penalty J r necnt terminal',
    'mpc_closed_loop_batch': 'A B H X0 horizon steps phase0 D d ndcnt q Pf tol max_iter return_traj offset qf terminal_rhs plant disturbance penalty J r necnt terminal',
    'mpc_step': 'A B Q R N x0 horizon phase0 D d q Pf tol max_iter offset qf terminal_rhs penalty J r terminal',
    'mpc_closed_loop_sim': 'A B Q R N x0 horizon steps phase0 D d q Pf tol max_iter offset qf terminal_rhs plant disturbance penalty J r terminal'}


def test_the_reported_signatures_of_the_four_calls_are_unchanged():
    from tunempc_amd import mpc_qp as m
    for name, want in SIGNATURES.items():
        f = getattr(m, name)
        sig = inspect.signature(f)
        assert list(sig.parameters) == want.split(), name
        assert not set(sig.parameters) & set(m.HIDDEN_KEYWORDS)
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
        assert f.__name__ == name and 'warm_floor' in f.__doc__ and 'penalty2' in f.__doc__
    assert m.HIDDEN_KEYWORDS == ('penalty2', 'guess', 'guess_shift', 'warm', 'warm_floor') and m.WARM_FLOOR == wr.WARM_FLOOR
    assert list(inspect.signature(m.mpc_closed_loop_plant).parameters) == 'A B H X0 horizon steps plant phase0 warm problem'.split()


# ----------------------------------------------------------------------------- 3. the C entries
def test_the_warm_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_mpc_qp_warm_batch_host', 'tmpc_mpc_qp_warm_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        f = getattr(lib, name)
        assert len(f.argtypes) == 60 and f.restype is C.c_int and f.argtypes[51] is C.c_int and f.argtypes[52] is C.c_double
        decl = header[header.index('int %s(' % name):]
        assert re.sub(r'\s+', ' ', decl[:decl.index(';')]).endswith(
            'const double* penalty2, int warm_flags, double warm_floor, const double* Xg, const double* Ug, const double* Lamg, const double* Eg, '
            'const double* Nug, const double* NuTg, int32_t* warmlog)')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_mpc_qp.h')).read()
    assert 'template <bool SOFT, bool EQ, bool AFF, bool QUAD, bool WARM = false>' in src and 'struct MpcQpWarm {' in src


def test_the_warm_entries_refuse_by_themselves_what_python_refuses():
    """TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call (this machine may have no device at all)."""
    from tunempc_amd._lib import load_library
    lib = load_library()
    d = (C.c_double * 64)(*([1.0] * 64))
    ok = dict(nb=1, p=2, nx=1, mb=1, nd=1, N=1, ns=1, T=1, k0=0, D=d, dd=d, tol=1e-10, it=60, A=d, U0=d, pen=None, pen2=None, flags=2, floor=1e-2, Xg=d, Ug=d, Lamg=d,
              Eg=None, Nug=None, NuTg=None, ne=0, J=None, nt=0)
    names = ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')
    for f, vp in ((lib.tmpc_mpc_qp_warm_batch_host, False), (lib.tmpc_mpc_qp_warm_batch_device, True)):
        P = (lambda x: C.cast(x, C.c_void_p) if x is not None else None) if vp else (lambda x: x)

        def call(**kw):
            a = {**ok, **kw}
            return f(*[a[k] for k in names], P(a['A']), P(d), P(d), None, None, P(a['D']), None, P(a['dd']), P(d), a['tol'], a['it'], P(a['U0']), P(d), P(d),
                     None, None, None, None, None, None, None, None, P(a['pen']), None, None, a['ne'], P(a['J']), None, None, a['nt'], None, None, None, None,
                     None, None, None, None, None, None, None, P(a['pen2']), a['flags'], a['floor'], P(a['Xg']), P(a['Ug']), P(a['Lamg']), P(a['Eg']), P(a['Nug']),
                     P(a['NuTg']), None)
        who = f.__name__.encode()
        for kw, txt in ((dict(nb=0), b'bad argument (nb, p'), (dict(k0=2), b'starting phase'), (dict(tol=0.0), b'tol > 0'), (dict(A=None), b'non-null A'),
                        (dict(flags=8), b'warm_flags'), (dict(flags=-1), b'warm_flags'), (dict(flags=4), b'warm_flags'), (dict(flags=5), b'warm_flags'),
                        (dict(flags=0), b'the guess arrays come exactly with bit 1'), (dict(flags=1), b'the guess arrays come exactly with bit 1'),
                        (dict(Xg=None), b'Xg and Ug at the least'), (dict(Ug=None), b'Xg and Ug at the least'),
                        (dict(Xg=None, Ug=None, Lamg=None), b'the guess arrays come exactly with bit 1'),
                        (dict(Eg=d), b'Eg only with penalty'), (dict(Nug=d), b'Nug only with equality rows'), (dict(NuTg=d), b'NuTg only with terminal rows'),
                        (dict(nd=0, D=None, dd=None), b'Lamg only with rows'),
                        (dict(floor=0.0), b'warm_floor > 0'), (dict(floor=-1.0), b'warm_floor > 0'), (dict(floor=float('inf')), b'warm_floor > 0'),
                        (dict(floor=float('nan')), b'warm_floor > 0'), (dict(pen2=d), b'penalty2 stands beside penalty')):
            assert call(**kw) == -1, kw
            msg = lib.tmpc_last_error()
            assert txt in msg and msg.startswith(who + b': '), (kw, msg)
        assert call(nx=40, mb=30) == -2 and b'nx + nu = 64' in lib.tmpc_last_error()
        assert call(nt=2) == -1 and b'nt = 2' in lib.tmpc_last_error()
