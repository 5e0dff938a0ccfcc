"""CPU tests of the eight MPC QP entries as one path (csrc/tmpc_api.hip: a call record, one check, one host and one device path): every instance of the shapes
of mpc_qp_entries_cases.py is solved by the numpy references (what test_gpu_mpc_qp_entries.py relies on), and what the entries refuse before a device is
touched is refused under the name of the entry that was called.  No device is needed: a call that reached the device here would return TMPC_E_HIP."""
import numpy as np
import pytest

import mpc_qp_affine_reference as af
import mpc_qp_entries_cases as ec

E_ARG = -1
ENTRIES = [(lv, wh) for lv in ec.LEVELS for wh in ec.WHERE]


@pytest.fixture(scope='module')
def lib():
    from tunempc_amd._lib import load_library
    return load_library()


def message(lib):
    return lib.tmpc_last_error().decode()


def problems():
    a = ec.shape_a()
    return [('a', a), ('a-penalty', dict(a, penalty=ec.penalty_of(a)))] + [('b-%s-%s' % (lv, n), P) for lv in ec.LEVELS for n, P in ec.variants(lv)]


@pytest.mark.parametrize('name,P', problems(), ids=[n for n, _ in problems()])
def test_every_instance_of_the_shapes_is_solved_by_the_reference(name, P):
    """Status 0 at every step of the loop on the polished solution, with its certificate; shape (a) has active rows at the outer states."""
    active = violated = 0
    for b in range(P['nb']):
        for s in range(P['ns']):
            r = af.closed_loop_aff(P['A'][b], P['B'][b], P['H'][b], P['N'], P['k0'], P['X0'][b, s], P['T'], None if P['penalty'] is None else P['penalty'][b],
                                   W=None if P['aff'] is None else P['aff'][6][b, s], **ec.reference_kwargs(P, b))
            print('   %s instance %d.%d: status %d steps %d margin %.1e nact %s nviol %s' % (name, b, s, r['status'], r['steps'], r['margin'], r['nact'], r['nviol']))
            assert r['status'] == 0 and r['steps'] == P['T'] and r['certificate'] and r['margin'] >= af.MARGIN_MIN
            active += int(r['nact'].sum()); violated += int(r['nviol'].sum())
    assert active >= 2 or not name.startswith('a')
    assert violated >= 1 or name != 'a-penalty'


# (level, the arguments next to an ndcnt out of range, whether the parent of this change already named the entry that was called: it passed the call on to the
# soft or hard entry when there were no rows and no affine array, and that entry reported the count)
NDCNT_CALLS = [('hard', {}, True), ('soft', {}, False), ('soft', dict(penalty='finite'), True), ('eq', {}, False), ('eq', dict(penalty='finite'), False),
               ('eq', dict(nt=-1), True), ('aff', {}, False), ('aff', dict(penalty='finite'), False), ('aff', dict(aff='offset'), True)]


@pytest.mark.parametrize('level,extra,held_before', NDCNT_CALLS, ids=['%s-%s' % (lv, '-'.join(sorted(e)) or 'plain') for lv, e, _ in NDCNT_CALLS])
def test_a_count_out_of_range_is_reported_by_the_host_entry_that_was_called(lib, level, extra, held_before):
    P = ec.shape_b()
    kw = dict(extra)
    if 'penalty' in kw:
        kw['penalty'] = ec.penalty_of(P)
    if 'aff' in kw:
        kw['aff'] = (np.zeros((2, 2, 2)),) + (None,) * 6
    rc, _ = ec.raw_call(lib, level, 'host', P, ndcnt=np.array([[2, 0], [0, 3]], np.int32), **kw)
    assert rc == E_ARG
    assert message(lib) == '%s: ndcnt[1][1] = 3 outside 0 .. nd = 2' % ec.symbol(level, 'host'), held_before


@pytest.mark.parametrize('level,where', ENTRIES, ids=['%s-%s' % e for e in ENTRIES])
def test_the_first_check_names_the_entry_that_was_called(lib, level, where):
    P = ec.variants(level)[0][1]
    rc, _ = ec.raw_call(lib, level, where, dict(P, nb=0), refused=True)
    assert rc == E_ARG
    assert message(lib).startswith(ec.symbol(level, where) + ': bad argument (nb, p, nx, nu, N, ns, T >= 1')
    rc, _ = ec.raw_call(lib, level, where, P, refused=True, k0=2)             # (every pointer given: the second check)
    assert rc == E_ARG
    assert message(lib) == ec.symbol(level, where) + ': bad argument (starting phase k0 in 0 .. p - 1 = 1; got 2)'


@pytest.mark.parametrize('level', ['eq', 'aff'])
def test_without_rows_the_ranges_are_still_checked_before_any_device_call(lib, level):
    """ne = 0, nt = 0 through the eq and aff host entries: a penalty of 0 or NaN, and counts of equality rows -- without J they are refused as such, with J
    (ne = 1) by their range."""
    P = ec.shape_b()
    who = ec.symbol(level, 'host')
    for bad, shown in ((0.0, '0'), (np.nan, 'nan')):
        pen = ec.penalty_of(P)
        pen[1, 0, 0] = bad
        rc, _ = ec.raw_call(lib, level, 'host', P, penalty=pen)
        assert rc == E_ARG and message(lib).endswith('penalty[1][0][0] = %s: > 0 expected (+inf: a hard row)' % shown), message(lib)
    rc, _ = ec.raw_call(lib, level, 'host', P, necnt=np.array([[1, 0], [0, 2]], np.int32))
    assert rc == E_ARG and message(lib).startswith(who + ': bad argument (J non-null exactly when ne > 0')
    rc, _ = ec.raw_call(lib, level, 'host', dict(P, **ec.shape_b_rows()), necnt=np.array([[1, 0], [0, 2]], np.int32))
    assert rc == E_ARG and message(lib) == who + ': necnt[1][1] = 2 outside 0 .. ne = 1'
