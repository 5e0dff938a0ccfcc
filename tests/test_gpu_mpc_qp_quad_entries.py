"""GPU tests of the two quad entries as C calls (raw ctypes on tmpc_mpc_qp_quad_batch_{host,device}; device pointers from torch tensors), with the NULL
combinations that tunempc_amd._lib never passes: penalty2 NULL (the aff entry with the same arguments, the same bits), every optional output left out, the
tails of the eq and aff levels absent or present, host against device.  Everything here is an equality of bits or an exact zero; the shapes are those of
mpc_qp_entries_cases.py (imported, not changed)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_entries_cases as ec  # noqa: E402

BASE = ec.REQUIRED + ec.OPTIONAL
TAIL = ec.TAIL_OUT['aff']


@functools.lru_cache(maxsize=None)
def library():
    from tunempc_amd._lib import load_library
    return load_library()


def quad_call(where, P, penalty2, omit=()):
    """One call of tmpc_mpc_qp_quad_batch_<where>: the argument list of mpc_qp_entries_cases.raw_call at the aff level, then penalty2.  Every output is passed
    pre-filled (NaN, integers -7) unless named in `omit` (NULL).  -> dict of the outputs as numpy arrays."""
    lib = library()
    names = BASE + TAIL
    outs = {k: np.full(sh, np.nan if dt is np.float64 else -7, dt) for k, (sh, dt) in ec.out_shapes(P).items() if k in names and k not in omit}
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
            return a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))
    o = lambda k: ptr(outs.get(k), k)
    args = [P[k] for k in ('nb', 'p', 'nx', 'mb', 'nd', 'N', 'ns', 'T', 'k0')] + [ptr(P[k]) for k in ('A', 'B', 'H', 'q', 'Pf', 'D', 'ndcnt', 'd', 'X0')] + [1e-10, 60]
    args += [o(k) for k in BASE]
    args += [ptr(P['penalty']), o('Eol'), o('nviol')]
    args += [P['ne'], ptr(P['J']), ptr(P['r']), ptr(P['necnt']), P['nt'], ptr(P['Tx']), o('Nu'), o('NuT'), o('eres')]
    args += [ptr(a) for a in (P['aff'] or (None,) * 7)]
    args += [ptr(penalty2)]
    if where == 'device':
        torch.cuda.synchronize()
    rc = getattr(lib, 'tmpc_mpc_qp_quad_batch_%s' % where)(*args)
    if where == 'device':
        torch.cuda.synchronize()
        outs = {k: (keep[k].cpu().numpy() if k in keep else v) for k, v in outs.items()}
    assert rc == 0, (where, rc, lib.tmpc_last_error().decode())
    return outs


def aff_call(where, P, **kw):
    rc, out = ec.raw_call(library(), 'aff', where, P, **kw)
    assert rc == 0, (where, rc, library().tmpc_last_error().decode())
    return out


def solved(out, P):
    return (out['info'][..., 0] == 0).all() and (out['info'][..., 1] == P['T']).all()


def weights(P, kind):
    """penalty, penalty2 on every row but the last of each stage (that one stays hard): L1 + L2, or pure quadratic."""
    pen = ec.penalty_of(P, 0.3 if kind == 'l12' else 0.0)
    pen2 = np.where(np.isfinite(pen), 2.0, 0.0)
    return pen, pen2


def problems():
    """(name, problem without penalties): the scalar shape, shape (b) plain, with equality rows and an affine tail, with the terminal constraint and its rhs."""
    b = ec.shape_b()
    rows, term = dict(b, **ec.shape_b_rows()), dict(b, nt=-1)
    return [('scalar', ec.shape_a()), ('plain', b), ('rows', rows), ('rows-aff', dict(rows, aff=ec.shape_b_affine(b, False))),
            ('terminal-aff', dict(term, aff=ec.shape_b_affine(b, True)))]


PROBLEMS = dict(problems())


def test_the_symbols_exist():
    lib = library()
    for where in ec.WHERE:
        f = getattr(lib, 'tmpc_mpc_qp_quad_batch_%s' % where)
        assert len(f.argtypes) == 51 and f.restype is C.c_int


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_without_penalty2_the_quad_entry_is_the_aff_entry(where, name):
    P = PROBLEMS[name]
    for Pp in (P, dict(P, penalty=ec.penalty_of(P))):
        aff, quad = aff_call(where, Pp), quad_call(where, Pp, None)
        assert solved(aff, Pp)
        assert not ec.same_bits(quad, aff, BASE + TAIL)


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_a_penalty2_of_zeros_is_the_aff_entry_with_the_penalty(where, name):
    P = PROBLEMS[name]
    Pp = dict(P, penalty=ec.penalty_of(P))
    aff, quad = aff_call(where, Pp), quad_call(where, Pp, np.zeros_like(Pp['penalty']))
    assert solved(aff, Pp)
    assert not ec.same_bits(quad, aff, BASE + TAIL)


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('kind', ['l12', 'pure'])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_every_optional_output_may_be_left_out(where, kind, name):
    P = PROBLEMS[name]
    pen, pen2 = weights(P, kind)
    Pp = dict(P, penalty=pen)
    full, short = quad_call(where, Pp, pen2), quad_call(where, Pp, pen2, omit=ec.OPTIONAL + TAIL)
    assert solved(full, Pp) and sorted(short) == sorted(ec.REQUIRED)
    assert not ec.same_bits(short, full, ec.REQUIRED)
    kept = [k for k in BASE + TAIL if full[k].dtype == np.float64 and np.isnan(full[k]).any() or full[k].dtype == np.int32 and (full[k] == -7).any()]
    assert not kept, kept                                                   # (no output of a full call keeps its fill)
    if not P['ne'] and not P['nt'] and P['aff'] is None:                     # the kernel without EQ does not write eres: zero by the header
        assert not (full['eres'].view(np.uint8) != 0).any() and full['Nu'].size == 0 and full['NuT'].size == 0
    hard = ~np.isfinite(pen)
    if P['ndcnt'] is None:
        assert (full['Eol'][:, :, :, hard[0, 0]] == 0).all() and (full['Eol'] >= 0).all()
    if kind == 'pure':                                                       # e = lam / Z on every pure row
        Z = np.where(pen2 > 0, pen2, 1.0)
        for b_ in range(P['nb']):
            for j in range(P['N']):
                k = (P['k0'] + j) % P['p']
                np.testing.assert_allclose(full['Eol'][b_, :, j], np.where(pen2[b_, k] > 0, full['Lam'][b_, :, j] / Z[b_, k], 0.0), rtol=0, atol=1e-15)


@pytest.mark.parametrize('kind', ['l12', 'pure'])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_the_host_and_the_device_entry_agree_bit_for_bit(kind, name):
    P = PROBLEMS[name]
    pen, pen2 = weights(P, kind)
    Pp = dict(P, penalty=pen)
    host, dev = quad_call('host', Pp, pen2), quad_call('device', Pp, pen2)
    assert solved(dev, Pp)
    assert not ec.same_bits(host, dev, BASE + TAIL)
