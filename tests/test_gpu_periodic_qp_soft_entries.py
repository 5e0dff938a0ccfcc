"""GPU tests of the C entries tmpc_periodic_qp_soft_batch_host / _device as a C caller sees them: NULL penalty, NULL penalty2 and both NULL (the bits of
the existing entry, zeros in Eps, nviol, pcost, emax), NULL optional outputs, counts outside their capacity clamped, the refusals with the entry's name in
tmpc_last_error, the two entries bit-equal and equal to the wrapper."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import periodic_qp_reference as pq  # noqa: E402
import periodic_qp_soft_reference as sq  # noqa: E402
from tunempc_amd import _lib, periodic_qp as lib_pq  # noqa: E402

OUT = ('X', 'U', 'Lam', 'Eps', 'Nu', 'Pi', 'nviol', 'info', 'res')
INS = ('A', 'B', 'H', 'q', 'offset', 'D', 'ndcnt', 'd', 'penalty', 'penalty2', 'J', 'r', 'necnt')


def raw(bt, device=False, outputs=OUT, tol=pq.TOL, max_iter=pq.MAX_ITER, sizes=None):
    """One call of the soft entry on the arrays of bt (None: NULL) -> (rc, dict of the outputs asked for as numpy arrays)."""
    lib = _lib.load_library()
    nb, p, nx, mb = bt['B'].shape
    nd = 0 if bt.get('D') is None else bt['D'].shape[2]
    ne = 0 if bt.get('J') is None else bt['J'].shape[2]
    if sizes:
        nd, ne = sizes.get('nd', nd), sizes.get('ne', ne)
    N = bt['periods'] * p
    shapes = dict(X=(nb, N, nx), U=(nb, N, mb), Lam=(nb, N, nd), Eps=(nb, N, nd), Nu=(nb, N, ne), Pi=(nb, N, nx), nviol=(nb,), info=(nb, 8), res=(nb, 6))
    ins = [bt.get(k) for k in INS]
    if device:
        ins = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ins]
        outs = {k: torch.full(shapes[k], -7, dtype=torch.int32 if k == 'nviol' else torch.float64, device='cuda') for k in outputs}
        ptr = lambda t: None if t is None or not t.numel() else C.c_void_p(t.data_ptr())
        torch.cuda.synchronize()
        fn = lib.tmpc_periodic_qp_soft_batch_device
    else:
        ins = [None if x is None else np.ascontiguousarray(x) for x in ins]
        outs = {k: np.full(shapes[k], -7, np.int32 if k == 'nviol' else np.float64) for k in outputs}
        ptr = lambda a: None if a is None or not a.size else (_lib._iptr(a) if a.dtype == np.int32 else _lib._dptr(a))
        fn = lib.tmpc_periodic_qp_soft_batch_host
    rc = fn(nb, p, nx, mb, nd, ne, bt['periods'], *[ptr(x) for x in ins], float(tol), int(max_iter), *[ptr(outs.get(k)) for k in OUT])
    return rc, {k: (v.cpu().numpy() if device else v) for k, v in outs.items()}


def test_host_and_device_entries_agree_bit_for_bit_and_with_the_wrapper():
    for cf in (sq.case_ragged, sq.case_contradictory, sq.case_wide_rows, sq.case_scalar_pure):
        bt = sq.batch_of(cf())
        rh, h = raw(bt)
        rd, d = raw(bt, device=True)
        assert rh == 0 and rd == 0
        for k in OUT:
            np.testing.assert_array_equal(h[k], d[k], err_msg=k)
        w = lib_pq.periodic_qp_batch(**bt)
        for a, b in (('X', 'X'), ('U', 'U'), ('Lam', 'lam'), ('Eps', 'eps'), ('Nu', 'nu'), ('Pi', 'pi'), ('nviol', 'nviol')):
            np.testing.assert_array_equal(h[a], w[b], err_msg=a)
        assert h['info'][0, 0] == 0 and h['info'][0, 1] == 1 and h['info'][0, 2] == h['info'][0, 3] == w['iters'][0]
        np.testing.assert_array_equal(h['res'][0], [w['cost'][0], w['hres'][0], w['eres'][0], w['per'][0], w['pcost'][0], w['emax'][0]])


def test_null_penalties():
    bt = sq.batch_of(sq.case_ragged())
    old = lib_pq.periodic_qp_batch(**pq.batch_of(pq.case_ragged()))
    for device in (False, True):
        # both NULL: the kernel of the existing entry, its bits, zeros in the rest
        rc, o = raw(dict(bt, penalty=None, penalty2=None), device)
        assert rc == 0
        for a, b in (('X', 'X'), ('U', 'U'), ('Lam', 'lam'), ('Nu', 'nu'), ('Pi', 'pi')):
            np.testing.assert_array_equal(o[a], old[b], err_msg=a)
        np.testing.assert_array_equal(o['res'][0], [old['cost'][0], old['hres'][0], old['eres'][0], old['per'][0], 0.0, 0.0])
        assert not o['Eps'].any() and not o['nviol'].any() and o['info'][0, 2] == old['iters'][0]
        # penalty2 NULL: Z = 0 (wide_rows: L1 rows only; beside a c = 0 a NULL penalty2 would be an invalid weight)
        l1 = sq.batch_of(sq.case_wide_rows())
        rc, o = raw(dict(l1, penalty2=None), device)
        rc0, z = raw(dict(l1, penalty2=np.zeros(l1['penalty'].shape)), device)
        assert rc == 0 and rc0 == 0 and o['info'][0, 0] == 0
        for k in OUT:
            np.testing.assert_array_equal(o[k], z[k], err_msg=k)
        # penalty NULL: every row pure quadratic
        zz = np.full(bt['penalty'].shape, 5.0)
        rc, o = raw(dict(bt, penalty=None, penalty2=zz), device)
        rc0, z = raw(dict(bt, penalty=np.zeros(zz.shape), penalty2=zz), device)
        assert rc == 0 and rc0 == 0 and o['info'][0, 0] == 0
        for k in OUT:
            np.testing.assert_array_equal(o[k], z[k], err_msg=k)
        np.testing.assert_array_equal(o['Eps'], o['Lam'] / 5.0)


def test_null_optional_outputs():
    bt = sq.batch_of(sq.case_wide_rows())
    full = raw(bt)[1]
    for device in (False, True):
        rc, o = raw(bt, device, outputs=('info',))                          # every optional output NULL
        assert rc == 0
        np.testing.assert_array_equal(o['info'], full['info'])
        rc, o = raw(bt, device, outputs=('Eps', 'info'))
        assert rc == 0
        np.testing.assert_array_equal(o['Eps'], full['Eps'])
        rc, o = raw(bt, device, outputs=('nviol', 'res', 'info'))
        assert rc == 0
        np.testing.assert_array_equal(o['nviol'], full['nviol']); np.testing.assert_array_equal(o['res'], full['res'])
        rc, o = raw(dict(bt, penalty=None, penalty2=None), device, outputs=('info',))      # ... and through the kernel of the existing entry
        assert rc == 0 and o['info'][0, 0] == 0


def test_counts_are_clamped():
    bt = sq.batch_of(sq.case_ragged())                                      # ndcnt 0 / 4 / 1 of nd = 4, necnt 1 / 0 / 0 of ne = 1
    ref = raw(bt)[1]
    wild = dict(bt, ndcnt=np.array([[-3, 9, 1]], np.int32), necnt=np.array([[5, -1, 0]], np.int32))
    for device in (False, True):
        rc, o = raw(wild, device)
        assert rc == 0
        for k in OUT:
            np.testing.assert_array_equal(o[k], ref[k], err_msg=k)


def test_refusals_before_the_device():
    lib = _lib.load_library()
    nx, nu = 40, 24
    nd = next(m for m in range(1, 4096) if lib_pq.lds_bytes(nx, nu, m, 0, True) > lib_pq.LDS_BYTES)
    big = dict(A=np.zeros((1, 1, nx, nx)), B=np.zeros((1, 1, nx, nu)), H=np.eye(nx + nu)[None, None], D=np.zeros((1, 1, nd, nx + nu)), d=np.ones((1, 1, nd)),
               penalty=np.ones((1, 1, nd)), periods=1)
    for device in (False, True):
        name = 'tmpc_periodic_qp_soft_batch_' + ('device' if device else 'host')
        rc, o = raw(big, device)
        msg = lib.tmpc_last_error().decode()
        assert rc == _lib.E_UNSUPPORTED and str(lib_pq.lds_bytes(nx, nu, nd, 0, True)) in msg and name in msg
        assert (o['info'] == -7.0).all()
        free = sq.batch_of(sq.case_scalar_l1())
        rc, _ = raw(dict(free, D=None, d=None), device)                     # nd = 0 with a penalty
        assert rc == -1 and name in lib.tmpc_last_error().decode() and 'nd = 0' in lib.tmpc_last_error().decode()
    bt = sq.batch_of(sq.case_ragged())
    for ch in (dict(d=None), dict(J=None), dict(periods=0)):
        rc, _ = raw(dict(bt, **ch), sizes=dict(nd=4, ne=1))
        assert rc == -1 and 'tmpc_periodic_qp_soft_batch_host' in lib.tmpc_last_error().decode(), ch
    assert raw(bt, tol=0.0)[0] == -1 and raw(bt, max_iter=0)[0] == -1
