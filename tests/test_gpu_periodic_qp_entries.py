"""GPU tests of the C entries tmpc_periodic_qp_batch_host / _device as a C caller sees them: NULL for every optional array, counts outside their capacity
clamped, TMPC_E_UNSUPPORTED beyond the LDS layout and TMPC_E_ARG before the device is touched, the two entries bit-equal."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import periodic_qp_reference as pq  # noqa: E402
from tunempc_amd import _lib, periodic_qp as lib_pq  # noqa: E402

OUT = ('X', 'U', 'Lam', 'Nu', 'Pi', 'info', 'res')


def raw(bt, device=False, outputs=OUT, tol=pq.TOL, max_iter=pq.MAX_ITER, sizes=None):
    """One call of the entry on the arrays of bt (None: NULL) -> (rc, dict of the outputs asked for as numpy arrays)."""
    lib = _lib.load_library()
    nb, p, nx, mb = bt['B'].shape
    nd = 0 if bt.get('D') is None else bt['D'].shape[2]
    ne = 0 if bt.get('J') is None else bt['J'].shape[2]
    if sizes:
        nd, ne = sizes.get('nd', nd), sizes.get('ne', ne)
    N = bt['periods'] * p
    shapes = dict(X=(nb, N, nx), U=(nb, N, mb), Lam=(nb, N, nd), Nu=(nb, N, ne), Pi=(nb, N, nx), info=(nb, 8), res=(nb, 4))
    ins = [bt.get(k) for k in ('A', 'B', 'H', 'q', 'offset', 'D', 'ndcnt', 'd', 'J', 'r', 'necnt')]
    if device:
        ins = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ins]
        outs = {k: torch.full(shapes[k], -7.0, dtype=torch.float64, device='cuda') for k in outputs}
        ptr = lambda t: None if t is None or not t.numel() else C.c_void_p(t.data_ptr())
        torch.cuda.synchronize()
        fn = lib.tmpc_periodic_qp_batch_device
    else:
        ins = [None if x is None else np.ascontiguousarray(x) for x in ins]
        outs = {k: np.full(shapes[k], -7.0) for k in outputs}
        ptr = lambda a: None if a is None or not a.size else (_lib._iptr(a) if a.dtype == np.int32 else _lib._dptr(a))
        fn = lib.tmpc_periodic_qp_batch_host
    rc = fn(nb, p, nx, mb, nd, ne, bt['periods'], *[ptr(x) for x in ins], float(tol), int(max_iter), *[ptr(outs.get(k)) for k in OUT])
    return rc, {k: (v.cpu().numpy() if device else v) for k, v in outs.items()}


def test_host_and_device_entries_agree_bit_for_bit_and_with_the_wrapper():
    for cf in (pq.case_ragged, pq.case_eig_one, pq.case_wide_rows):
        bt = pq.batch_of(cf())
        rh, h = raw(bt)
        rd, d = raw(bt, device=True)
        assert rh == 0 and rd == 0
        for k in OUT:
            np.testing.assert_array_equal(h[k], d[k], err_msg=k)
        w = lib_pq.periodic_qp_batch(**bt)
        for a, b in (('X', 'X'), ('U', 'U'), ('Lam', 'lam'), ('Nu', 'nu'), ('Pi', 'pi')):
            np.testing.assert_array_equal(h[a], w[b], err_msg=a)
        assert h['info'][0, 0] == 0 and h['info'][0, 1] == 1 and h['info'][0, 2] == h['info'][0, 3] == w['iters'][0]
        np.testing.assert_array_equal(h['res'][0], [w['cost'][0], w['hres'][0], w['eres'][0], w['per'][0]])


def test_null_optionals():
    c = pq.case_scalar_free()
    bt = pq.batch_of(c)
    full = raw(bt)[1]
    for device in (False, True):
        rc, o = raw(bt, device, outputs=('info',))                          # every optional output NULL
        assert rc == 0
        np.testing.assert_array_equal(o['info'], full['info'])
        rc, o = raw(bt, device, outputs=('X', 'info'))
        assert rc == 0
        np.testing.assert_array_equal(o['X'], full['X'])
        # every optional input NULL: q = 0, c = 0, no rows -- the orbit of the homogeneous problem is the origin
        rc, o = raw(dict(A=bt['A'], B=bt['B'], H=bt['H'], periods=1), device)
        assert rc == 0 and o['info'][0, 0] == 0 and not o['X'].any() and not o['U'].any() and o['res'][0, 1] == -np.inf
    # r NULL is r = 0, ndcnt / necnt NULL is every row
    rg = pq.batch_of(pq.case_odd())
    zero_r = dict(rg, r=np.zeros_like(rg['r']))
    np.testing.assert_array_equal(raw(dict(rg, r=None))[1]['X'], raw(zero_r)[1]['X'])
    bx = pq.batch_of(pq.case_unstable())
    allrows = dict(bx, ndcnt=np.full(bx['D'].shape[:2], bx['D'].shape[2], np.int32))
    np.testing.assert_array_equal(raw(bx)[1]['X'], raw(allrows)[1]['X'])


def test_counts_are_clamped():
    bt = pq.batch_of(pq.case_ragged())                                      # ndcnt 0 / 4 / 1 of nd = 4, necnt 1 / 0 / 0 of ne = 1
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
    big = dict(A=np.zeros((1, 1, nx, nx)), B=np.zeros((1, 1, nx, nu)), H=np.eye(nx + nu)[None, None], D=np.zeros((1, 1, 64, nx + nu)), d=np.ones((1, 1, 64)),
               J=np.zeros((1, 1, 8, nx + nu)), periods=1)
    for device in (False, True):
        rc, o = raw(big, device)
        msg = lib.tmpc_last_error().decode()
        assert rc == _lib.E_UNSUPPORTED and str(lib_pq.lds_bytes(nx, nu, 64, 8)) in msg and 'tmpc_periodic_qp_batch_' + ('device' if device else 'host') in msg
        assert (o['info'] == -7.0).all()
    bt = pq.batch_of(pq.case_ragged())
    for ch in (dict(d=None), dict(J=None), dict(periods=0)):
        rc, _ = raw(dict(bt, **ch), sizes=dict(nd=4, ne=1))
        assert rc == -1, ch
    assert raw(bt, tol=0.0)[0] == -1 and raw(bt, max_iter=0)[0] == -1
    wide = dict(A=np.zeros((1, 1, 60, 60)), B=np.zeros((1, 1, 60, 5)), H=np.eye(65)[None, None], periods=1)
    assert raw(wide)[0] == _lib.E_UNSUPPORTED
