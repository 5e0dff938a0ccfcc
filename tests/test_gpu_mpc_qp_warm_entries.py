"""GPU tests of the two warm entries as C calls (raw ctypes on tmpc_mpc_qp_warm_batch_{host,device}; device pointers from torch tensors), with the NULL
combinations that tunempc_amd._lib never passes: warm_flags = 0 (the quad / aff entry with the same arguments, the same bits, warmlog zero), warmlog left out,
a guess of X and U alone (the multipliers NULL: zeros before the floors), every optional output left out, host against device.  Equalities of bits, exact
zeros and log codes; the shapes are those of mpc_qp_entries_cases.py (imported, not changed)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_entries_cases as ec  # noqa: E402

BASE = ec.REQUIRED + ec.OPTIONAL
TAIL = ec.TAIL_OUT['aff']
GUESS = ('Xol', 'Uol', 'Lam', 'Eol', 'Nu', 'NuT')


@functools.lru_cache(maxsize=None)
def library():
    from tunempc_amd._lib import load_library
    return load_library()


def warm_call(where, P, flags=0, floor=1e-2, guess=(None,) * 6, penalty2=None, omit=(), log=True):
    """One call of tmpc_mpc_qp_warm_batch_<where>: the argument list of the quad entry, then warm_flags, warm_floor, the six guess arrays (None: NULL) and
    warmlog (log False: NULL).  Every output is passed pre-filled (NaN, integers -7) unless named in `omit` (NULL).  -> dict of the outputs as numpy arrays."""
    lib = library()
    names = BASE + TAIL
    outs = {k: np.full(sh, np.nan if dt is np.float64 else -7, dt) for k, (sh, dt) in ec.out_shapes(P).items() if k in names and k not in omit}
    if log:
        outs['warmlog'] = np.full((P['nb'], P['T'], P['ns']), -7, np.int32)
    keep = {}
    if where == 'device':
        def ptr(a, name=None):
            if a is None or not a.size:
                return None
            keep[name or len(keep)] = t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return C.c_void_p(t.data_ptr())
    else:
        def ptr(a, name=None):
            if a is None or not a.size:
                return None
            a = np.ascontiguousarray(a)
            keep[name or len(keep)] = a
            return a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))
    o = lambda k: ptr(outs.get(k), k)
    args = [P[k] for k in ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')] + [ptr(P[k]) for k in ('A', 'B', 'H', 'q', 'Pf', 'D', 'ndcnt', 'd', 'X0')] + [1e-10, 60]
    args += [o(k) for k in BASE]
    args += [ptr(P['penalty']), o('Eol'), o('nviol')]
    args += [P['ne'], ptr(P['J']), ptr(P['r']), ptr(P['necnt']), P['nt'], ptr(P['Tx']), o('Nu'), o('NuT'), o('eres')]
    args += [ptr(a) for a in (P['aff'] or (None,) * 7)]
    args += [ptr(penalty2), int(flags), float(floor)] + [ptr(g) for g in guess] + [o('warmlog')]
    if where == 'device':
        torch.cuda.synchronize()
    rc = getattr(lib, 'tmpc_mpc_qp_warm_batch_%s' % where)(*args)
    if where == 'device':
        torch.cuda.synchronize()
        outs = {k: (keep[k].cpu().numpy() if k in keep else v) for k, v in outs.items()}
    else:
        outs = {k: (keep[k] if k in keep else v) for k, v in outs.items()}
    assert rc == 0, (where, rc, lib.tmpc_last_error().decode())
    return outs


def aff_call(where, P):
    rc, out = ec.raw_call(library(), 'aff', where, P)
    assert rc == 0, (where, rc, library().tmpc_last_error().decode())
    return out


def solved(out, P):
    return (out['info'][..., 0] == 0).all() and (out['info'][..., 1] == P['T']).all()


def problems():
    b = ec.shape_b()
    rows, term = dict(b, **ec.shape_b_rows()), dict(b, nt=-1)
    return [('scalar', ec.shape_a()), ('plain', b), ('plain-penalty', dict(b, penalty=ec.penalty_of(b))), ('rows-aff', dict(rows, aff=ec.shape_b_affine(b, False))),
            ('terminal-aff', dict(term, aff=ec.shape_b_affine(b, True)))]


PROBLEMS = dict(problems())


def guess_from(out, P, keys=GUESS):
    """The guess arguments from the outputs of an earlier call: Eol only with penalty, Nu / NuT only with rows (the entry refuses them otherwise)."""
    have = dict(Xol=True, Uol=True, Lam=P['nd'] > 0, Eol=P['penalty'] is not None, Nu=P['ne'] > 0, NuT=P['nt'] != 0)
    return tuple(out[k] if have[k] and k in keys else None for k in GUESS)


def test_the_symbols_exist():
    lib = library()
    for where in ec.WHERE:
        f = getattr(lib, 'tmpc_mpc_qp_warm_batch_%s' % where)
        assert len(f.argtypes) == 60 and f.restype is C.c_int


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_without_flags_the_warm_entry_is_the_aff_entry(where, name):
    P = PROBLEMS[name]
    aff, warm = aff_call(where, P), warm_call(where, P)
    assert solved(aff, P)
    assert not ec.same_bits(warm, aff, BASE + TAIL)
    assert not warm['warmlog'].any()                                         # every step cold: zero by the header
    assert not ec.same_bits(warm_call(where, P, log=False), aff, BASE + TAIL)


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_warm_loop_and_guess_through_the_raw_entry(where, name):
    P = PROBLEMS[name]
    cold = warm_call(where, P)
    loop = warm_call(where, P, flags=1)
    assert solved(loop, P)
    assert (loop['warmlog'][:, 0] == 0).all() and np.isin(loop['warmlog'][:, 1:], (1, 2)).all()
    assert not ec.same_bits(loop, cold, ('Xol', 'Uol', 'Lam', 'U0'))          # step 0 is the cold step
    assert np.abs(loop['X'] - cold['X']).max() <= 1e-7 and (loop['nact'] == cold['nact']).all()
    short = warm_call(where, P, flags=1, omit=ec.OPTIONAL + TAIL, log=False)
    assert sorted(short) == sorted(ec.REQUIRED) and not ec.same_bits(short, loop, ec.REQUIRED)
    # the guess: the solution of the cold call for the same phase; with every array the problem has, and with X and U alone
    full = warm_call(where, P, flags=3, guess=guess_from(cold, P))
    bare = warm_call(where, P, flags=3, guess=guess_from(cold, P, ('Xol', 'Uol')))
    for out in (full, bare):
        assert solved(out, P) and np.isin(out['warmlog'], (1, 2)).all()
        assert np.abs(out['X'] - cold['X']).max() <= 1e-7 and np.abs(out['Uol'] - cold['Uol']).max() <= 1e-7
    assert int(full['iters'][:, 0].sum()) < int(cold['iters'][:, 0].sum())   # started at the solution
    kept = [k for k in BASE + TAIL + ('warmlog',) if full[k].dtype == np.float64 and np.isnan(full[k]).any() or full[k].dtype == np.int32 and (full[k] == -7).any()]
    assert not kept, kept
    shifted = warm_call(where, P, flags=7, guess=guess_from(cold, P))
    assert solved(shifted, P) and np.isin(shifted['warmlog'], (1, 2)).all() and np.abs(shifted['X'] - cold['X']).max() <= 1e-7


@pytest.mark.parametrize('name', list(PROBLEMS))
def test_the_host_and_the_device_entry_agree_bit_for_bit(name):
    P = PROBLEMS[name]
    cold = warm_call('host', P)
    for flags, guess in ((1, (None,) * 6), (3, guess_from(cold, P)), (7, guess_from(cold, P, ('Xol', 'Uol', 'Lam')))):
        host, dev = warm_call('host', P, flags, guess=guess), warm_call('device', P, flags, guess=guess)
        assert solved(dev, P)
        assert not ec.same_bits(host, dev, BASE + TAIL + ('warmlog',))
