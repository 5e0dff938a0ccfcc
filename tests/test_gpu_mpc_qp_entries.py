"""GPU tests of the eight MPC QP entries as C calls (raw ctypes on tmpc_mpc_qp_*_batch_{host,device}; device pointers from torch tensors): the promises of
include/tunempc_hip.h that tunempc_amd._lib never exercises, because it passes Eol / nviol only with a penalty and never leaves iters / nact / hres out --
outputs that the kernel of a call does not write are zero, an entry without the arguments of its level gives the bits of the entry below, every optional output
may be NULL, and the host and the device entry agree bit for bit.  Everything here is an equality of bits or an exact zero; the shapes are those of
mpc_qp_entries_cases.py, solved by the numpy references in test_mpc_qp_entries_cpu.py."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library is loaded)

pytestmark = pytest.mark.gpu

import mpc_qp_entries_cases as ec  # noqa: E402

BASE = ec.REQUIRED + ec.OPTIONAL


@functools.lru_cache(maxsize=None)
def library():
    from tunempc_amd._lib import load_library
    return load_library()


def plain_shapes():
    """Shape (a) and shape (b) without equality rows: the problems of the hard and soft entries."""
    return dict(a=ec.shape_a(), b=ec.shape_b())


def call(level, where, P, **kw):
    rc, out = ec.raw_call(library(), level, where, P, **kw)
    assert rc == 0, (level, where, rc, library().tmpc_last_error().decode())
    return out


def solved(out, P):
    return (out['info'][..., 0] == 0).all() and (out['info'][..., 1] == P['T']).all()


def all_zero(out, keys):
    return [k for k in keys if out[k].size and (out[k].view(np.uint8) != 0).any()]


# ----------------------------------------------------------------------------- 1. / 2. without the arguments of its level an entry is the entry below
@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('shape', ['a', 'b'])
def test_the_soft_entry_without_penalty_is_the_hard_entry_and_zeroes_its_outputs(where, shape):
    P = plain_shapes()[shape]
    hard, soft = call('hard', where, P), call('soft', where, P)
    assert solved(hard, P) and (hard['nact'] > 0).any() == (shape == 'a')
    assert not all_zero(soft, ('Eol', 'nviol'))
    assert not ec.same_bits(soft, hard, BASE)


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('shape', ['a', 'b'])
def test_the_eq_entry_without_rows_is_the_hard_or_soft_entry_and_zeroes_its_outputs(where, shape):
    P = plain_shapes()[shape]
    hard, eq = call('hard', where, P), call('eq', where, P)
    assert not all_zero(eq, ('Eol', 'nviol', 'eres'))
    assert eq['Nu'].size == 0 and eq['NuT'].size == 0
    assert not ec.same_bits(eq, hard, BASE)
    Ps = dict(P, penalty=ec.penalty_of(P))
    soft, eqs = call('soft', where, Ps), call('eq', where, Ps)
    assert solved(soft, Ps) and (shape != 'a' or (soft['nviol'] > 0).any())
    assert not all_zero(eqs, ('eres',))
    assert not ec.same_bits(eqs, soft, BASE + ('Eol', 'nviol'))


# ----------------------------------------------------------------------------- 3. the EQ kernels without penalty do not write Eol, nviol
@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('name', ['rows', 'terminal'])
def test_the_eq_entry_with_rows_and_no_penalty_zeroes_Eol_and_nviol(where, name):
    P = dict(ec.variants('eq'))[name]
    full, without = call('eq', where, P), call('eq', where, P, omit=('Eol', 'nviol'))
    assert solved(full, P)
    assert not all_zero(full, ('Eol', 'nviol'))
    assert not ec.same_bits(full, without, BASE + ('Nu', 'NuT', 'eres'))
    assert np.isfinite(full['Nu']).all() and np.isfinite(full['NuT']).all() and np.isfinite(full['eres']).all()
    assert (full['Nu'] != 0).any() if name == 'rows' else (full['NuT'] != 0).any()


# ----------------------------------------------------------------------------- 4. every optional output may be NULL
ENTRY_VARIANTS = [(lv, n) for lv in ec.LEVELS for n, _ in ec.variants(lv)]


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('level,name', ENTRY_VARIANTS, ids=['%s-%s' % e for e in ENTRY_VARIANTS])
def test_every_optional_output_may_be_left_out(where, level, name):
    P = dict(ec.variants(level))[name]
    full, short = call(level, where, P), call(level, where, P, omit=ec.OPTIONAL + ec.TAIL_OUT[level])
    assert solved(full, P) and sorted(short) == sorted(ec.REQUIRED)
    assert not ec.same_bits(short, full, ec.REQUIRED)
    kept = [k for k in BASE + ec.TAIL_OUT[level] if full[k].dtype == np.float64 and np.isnan(full[k]).any() or full[k].dtype == np.int32 and (full[k] == -7).any()]
    assert not kept, kept                                                   # (no output of a full call keeps its fill)


@pytest.mark.parametrize('where', ec.WHERE)
@pytest.mark.parametrize('level', ['hard', 'soft'])
def test_every_optional_output_may_be_left_out_at_the_scalar_shape(where, level):
    P = ec.shape_a()
    P = P if level == 'hard' else dict(P, penalty=ec.penalty_of(P))
    full, short = call(level, where, P), call(level, where, P, omit=ec.OPTIONAL + ec.TAIL_OUT[level])
    assert solved(full, P) and not ec.same_bits(short, full, ec.REQUIRED)


# ----------------------------------------------------------------------------- 5. host against device
@pytest.mark.parametrize('level,name', ENTRY_VARIANTS, ids=['%s-%s' % e for e in ENTRY_VARIANTS])
def test_the_host_and_the_device_entry_agree_bit_for_bit(level, name):
    P = dict(ec.variants(level))[name]
    host, dev = call(level, 'host', P), call(level, 'device', P)
    assert solved(dev, P)
    assert not ec.same_bits(host, dev, BASE + ec.TAIL_OUT[level])
