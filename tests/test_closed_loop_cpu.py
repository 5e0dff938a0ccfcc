"""CPU tests of the closed-loop rollout: the numpy reference against itself (tests/closed_loop_reference.py), the figures that bound the GPU tests, and what
tunempc_amd.closed_loop refuses before it loads the library.  No device is needed."""
import os
import re

import numpy as np
import pytest

import closed_loop_reference as cr
import lqr_horizon_reference as lh

# The figures of the numpy reference, asserted below and imported by test_gpu_closed_loop.py.
TELESCOPING_DEFECT_REL = 1e-15       # measured: 1.3e-16, 4.5e-17, 5.2e-16, 6.7e-17 on the four cases (random K, T = 2p + 1, phase0 = p - 1)
MONODROMY_DISAGREEMENT = 1e-15       # rollout of I against the explicit product, relative to max(1, max|Phi|); measured: at most 3.6e-16
RHO_RAGGED = {1: 0.38929, 2: 0.16284, 5: 0.079202, 8: 0.077887, 30: 0.077879}      # receding-horizon rho of case_ragged_rows, Hc side, terminal cost


@pytest.mark.parametrize('case', cr.CASES, ids=[c.__name__ for c in cr.CASES])
def test_telescoping_identity_of_the_reference(case):
    d = cr.with_feedback(case)
    p = d['A'].shape[0]
    defect, rel = cr.telescoping_defect(d['A'], d['B'], d['H'], d['Hc'], d['P'], d['K'], d['X0'], 2 * p + 1, p - 1)
    print('   %s: defect %s  defect_rel %s' % (case.__name__, defect, rel))
    assert rel.max() <= TELESCOPING_DEFECT_REL
    # the contrast: without the phase shift of P the identity does not hold (p > 1), so the test can fail
    if p > 1:
        r = cr.rollout(d['A'], d['B'], d['K'], d['X0'], 2 * p + 1, p - 1, H=d['H'], Hc=d['Hc'])
        wrong = 0.5 * np.einsum('si,ij,sj->s', r['XT'], d['P'][p - 1], r['XT']) - 0.5 * np.einsum('si,ij,sj->s', d['X0'], d['P'][p - 1], d['X0'])
        assert np.abs(r['Lc'] - r['L'] - wrong).max() > 1e-3


@pytest.mark.parametrize('case', cr.CASES, ids=[c.__name__ for c in cr.CASES])
def test_monodromy_two_ways(case):
    d = cr.with_feedback(case)
    roll = cr.monodromy_rollout(d['A'], d['B'], d['K']); prod = cr.monodromy_product(d['A'], d['B'], d['K'])
    e = np.abs(roll - prod).max() / max(1.0, np.abs(prod).max())
    print('   %s: disagreement %.2e  rho %.4f' % (case.__name__, e, cr.rho(prod)))
    assert e <= MONODROMY_DISAGREEMENT
    nx = d['A'].shape[1]
    Pz = np.eye(nx); Pz[0, 0] = 0.0
    e = np.abs(cr.monodromy_rollout(d['A'], d['B'], d['K'], Pz) - prod @ Pz).max() / max(1.0, np.abs(prod).max())
    assert e <= MONODROMY_DISAGREEMENT


def test_receding_horizon_rho_decreases_to_the_periodic_value():
    c = lh.case_ragged_rows()
    got = {N: cr.receding_horizon(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], N, 'cost', None) for N in RHO_RAGGED}
    print({N: (r['rho'], r['subres']) for N, r in got.items()})
    Ns = sorted(RHO_RAGGED)
    for N in Ns:
        assert abs(got[N]['rho'] - RHO_RAGGED[N]) <= 5e-4 * RHO_RAGGED[N], N      # three digits
        assert got[N]['subres'] <= 1e-12
    assert all(got[a]['rho'] > got[b]['rho'] for a, b in zip(Ns, Ns[1:]))
    assert abs(got[30]['rho'] - got[8]['rho']) <= 1e-5 and abs(got[8]['rho'] - got[5]['rho']) > 1e-4
    c = lh.case_no_feasible_subspace()
    args = (c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0])
    assert cr.receding_horizon(*args, 4)['infeasible'] and not cr.receding_horizon(*args, 1)['infeasible']


def test_the_rollout_reference_wraps_the_phase_and_honours_ragged_rows():
    d = cr.with_feedback(lh.case_ragged_rows)
    r = cr.rollout(d['A'], d['B'], d['K'], d['X0'], 7, 2, H=d['H'], J=d['J'], rows=d['rows'], Hn=d['Hn'])
    x = d['X0'][1]
    for t in range(7):
        k = (2 + t) % 3
        u = -d['K'][k] @ x
        z = np.concatenate([x, u])
        assert np.allclose(r['U'][1, t], u, rtol=0, atol=1e-12 * max(1, np.abs(u).max()))
        assert np.isclose(r['l'][1, t], 0.5 * z @ d['H'][k] @ z, rtol=1e-12)
        rk = int(d['rows'][k])
        assert np.isclose(r['rowres'][1, t], np.abs(d['J'][k, :rk] @ z).max() if rk else 0.0, rtol=1e-12, atol=0)
        x = d['A'][k] @ x + d['B'][k] @ u
    assert np.allclose(r['XT'][1], x, rtol=1e-12)


# ----------------------------------------------------------------------------- validation without a device, and without the library
def _batch(nb=2, p=3, nx=4, mb=2, ns=5):
    return np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, mb)), np.zeros((nb, p, mb, nx)), np.zeros((nb, ns, nx))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test."""
    from tunempc_amd import _lib

    def refuse():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load_library', refuse)


def test_argument_checks_happen_before_the_library_is_loaded(no_library):
    from tunempc_amd import closed_loop as cl
    A, B, K, X0 = _batch()
    H = np.zeros((2, 3, 6, 6))
    for bad in (0, -2, 1.0, True, None):
        with pytest.raises(ValueError, match='steps must be an int >= 1'):
            cl.closed_loop_batch(A, B, K, X0, bad)
    for bad in (-1, 3, 0.0, None, True):
        with pytest.raises(ValueError, match='phase0 must be an int in 0 .. p - 1 = 2'):
            cl.closed_loop_batch(A, B, K, X0, 4, phase0=bad)
    with pytest.raises(ValueError, match='ns >= 1 initial states expected'):
        cl.closed_loop_batch(A, B, K, np.zeros((2, 0, 4)), 4)
    with pytest.raises(ValueError, match='X0 \\[nb, ns, nx\\] = \\[2, ns, 4\\] expected'):
        cl.closed_loop_batch(A, B, K, np.zeros((2, 5, 3)), 4)
    with pytest.raises(ValueError, match='K \\[nb, p, nu, nx\\] = \\(2, 3, 2, 4\\) expected'):
        cl.closed_loop_batch(A, B, np.zeros((2, 3, 4, 2)), X0, 4)
    with pytest.raises(ValueError, match='A \\[nb, p, nx, nx\\] expected'):
        cl.closed_loop_batch(A[0], B, K, X0, 4)
    with pytest.raises(ValueError, match='B \\[nb, p, nx, nu\\]'):
        cl.closed_loop_batch(A, B[:, :2], K, X0, 4)
    with pytest.raises(ValueError, match='fp64 arrays expected \\(K has dtype float32\\)'):
        cl.closed_loop_batch(A, B, K.astype(np.float32), X0, 4)
    with pytest.raises(ValueError, match='H \\(2, 3, 6, 6\\) expected'):
        cl.closed_loop_batch(A, B, K, X0, 4, H=np.zeros((2, 3, 6, 5)))
    with pytest.raises(ValueError, match='Hc \\(2, 3, 6, 6\\) expected'):
        cl.closed_loop_batch(A, B, K, X0, 4, H=H, Hc=np.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError, match='Hn \\(2, 3, 4, 4\\) expected'):
        cl.closed_loop_batch(A, B, K, X0, 4, Hn=np.zeros((2, 3, 2, 4)))
    with pytest.raises(ValueError, match='closed_loop_batch: ncnt / ng describe the rows of J, which is None'):
        cl.closed_loop_batch(A, B, K, X0, 4, ng=1)
    with pytest.raises(ValueError, match='closed_loop_batch: ncnt / ng describe the rows of J, which is None'):
        cl.closed_loop_batch(A, B, K, X0, 4, ncnt=np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match='closed_loop_batch: J \\[nb, p, nr, nx \\+ nu\\]'):
        cl.closed_loop_batch(A, B, K, X0, 4, J=np.zeros((2, 3, 1, 5)))
    with pytest.raises(ValueError, match='ng <= J.shape\\[2\\] = 1 expected, got 2'):
        cl.closed_loop_batch(A, B, K, X0, 4, J=np.zeros((2, 3, 1, 6)), ng=2)
    with pytest.raises(ValueError, match='closed_loop_monodromy_batch: Pz0 \\[nb, nx, nx\\]'):
        cl.closed_loop_monodromy_batch(A, B, K, Pz0=np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match='closed_loop_monodromy_batch: K \\[nb, p, nu, nx\\]'):
        cl.closed_loop_monodromy_batch(A, B, K[:, :, :1])
    with pytest.raises(ValueError, match='cost_equivalence_batch: P \\(2, 3, 4, 4\\) expected'):
        cl.cost_equivalence_batch(A, B, H, H, np.zeros((2, 3, 4, 3)), K, X0, 4)
    with pytest.raises(ValueError, match='cost_equivalence_batch: Hc must be an array'):
        cl.cost_equivalence_batch(A, B, H, None, A, K, X0, 4)
    with pytest.raises(ValueError, match='cost_equivalence_batch: steps must be an int >= 1'):
        cl.cost_equivalence_batch(A, B, H, H, A, K, X0, 0)
    with pytest.raises(ValueError, match='horizons must be a non-empty list of ints >= 1'):
        cl.horizon_closed_loop_batch(A, B, H, [0, 2])
    args = (np.eye(2), np.ones((2, 1)))
    with pytest.raises(ValueError, match='closed_loop_sim: K must be one \\(nu, nx\\) matrix or a list of p = 1 of them'):
        cl.closed_loop_sim(*args, np.zeros((2, 1)), np.ones(2), 3)
    with pytest.raises(ValueError, match='closed_loop_sim: x0 must hold nx = 2 entries'):
        cl.closed_loop_sim(*args, np.zeros((1, 2)), np.ones(3), 3)
    with pytest.raises(ValueError, match='closed_loop_sim: dHc must hold p matrices'):
        cl.closed_loop_sim(*args, np.zeros((1, 2)), np.ones(2), 3, dHc=[np.zeros((2, 2))])


def test_mixed_numpy_and_torch_arguments_are_refused(no_library):
    import torch
    from tunempc_amd import closed_loop as cl
    A, B, K, X0 = _batch()
    t = lambda x: torch.zeros(x.shape, dtype=torch.float64)
    with pytest.raises(ValueError, match='closed_loop_batch: the arrays must be all numpy arrays or all torch tensors \\(K differs\\)'):
        cl.closed_loop_batch(A, B, t(K), X0, 4)
    with pytest.raises(ValueError, match='all numpy arrays or all torch tensors \\(Hn differs\\)'):
        cl.closed_loop_batch(A, B, K, X0, 4, Hn=t(A))
    with pytest.raises(ValueError, match='J must be a numpy array like A, B, H'):
        cl.closed_loop_batch(A, B, K, X0, 4, J=torch.zeros((2, 3, 1, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match='torch tensors must be float64 tensors of one GPU'):
        cl.closed_loop_batch(t(A), t(B), t(K), t(X0), 4)                     # (torch tensors, but in host memory)
    with pytest.raises(ValueError, match='closed_loop_monodromy_batch: the arrays must be all numpy arrays or all torch tensors \\(Pz0 differs\\)'):
        cl.closed_loop_monodromy_batch(A, B, K, Pz0=torch.zeros((2, 4, 4), dtype=torch.float64))


def test_shapes_beyond_the_layout_are_refused_before_the_library_is_loaded(no_library):
    from tunempc_amd import closed_loop as cl
    z = np.zeros
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64 \\(got 70\\)'):
        cl.closed_loop_batch(z((1, 2, 40, 40)), z((1, 2, 40, 30)), z((1, 2, 30, 40)), z((1, 1, 40)), 3)
    with pytest.raises(NotImplementedError, match='nx = 32, nu = 32 with room for 200 rows per stage needs \\d+ bytes of LDS for a single state \\(limit 163840\\)'):
        cl.closed_loop_batch(z((1, 2, 32, 32)), z((1, 2, 32, 32)), z((1, 2, 32, 32)), z((1, 1, 32)), 3, J=z((1, 2, 200, 64)))


def _ctg_bytes(nx, mb, nr):
    """lqr_ctg_lds of csrc/tmpc_lqr_ctg.h restated (as in test_lqr_horizon_cpu.py) -> bytes."""
    n = nx + mb
    nbd, ms = min(mb, nr + nx), max(nr + nx, mb)
    ld, ldp, ldc = (n + nbd) | 1, nx | 1, n | 1
    return 8 * (nx * ld + nx * ldp + max(nx, mb + nbd) * ld + (n + nbd) * ld + 2 * ms * ldc + 2 * nx * ldp + 16)


def test_the_layout_serves_every_stage_block_and_the_rows_the_ctg_layout_serves():
    from tunempc_amd import closed_loop as cl
    for sh in ((24, 8, 10), (40, 24, 0), (1, 1, 0)):
        lay = cl.lds_layout(*sh)
        assert lay['ts'] >= 1 and lay['bytes'] <= 160 * 1024, (sh, lay)
    assert cl.lds_layout(24, 8, 10)['ts'] == 64 and cl.lds_layout(24, 8, 10)['bytes'] <= 80 * 1024      # two workgroups per CU at the bench stage shape
    assert cl.lds_layout(40, 24, 0)['ts'] == 32
    for n in range(2, 65):
        for nx in range(1, n):
            mb = n - nx
            lay = cl.lds_layout(nx, mb, 0)
            assert lay['ts'] >= 8 and lay['ts'] & (lay['ts'] - 1) == 0 and lay['bytes'] <= 160 * 1024, (nx, mb, lay)
            for nr in (1, 5, 16, 40, 66, 130):
                if _ctg_bytes(nx, mb, nr) <= 160 * 1024:
                    lay = cl.lds_layout(nx, mb, nr)
                    assert lay['ts'] >= 8 and lay['bytes'] <= 160 * 1024, (nx, mb, nr, lay)


def test_the_layout_of_the_kernel_header_is_the_one_restated_in_python():
    """The terms of closed_loop_lds in csrc/tmpc_closed_loop.h, read from the source: the buffers, the 80 KB rule for TS = 64 and the budget."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    src = open(os.path.join(root, 'tunempc_amd', 'csrc', 'tmpc_closed_loop.h')).read()
    body = src[src.index('inline ClosedLoopLds closed_loop_lds'):src.index('// Four rows')]
    for term in ('l.oK = l.oE + nx * l.ldn', 'l.oM = l.oK + mb * l.ldx', 'l.oJ = l.oM + n * l.ldn', 'l.oN = l.oJ + nr * l.ldn', 'l.oP = l.oN + nx * l.ldx',
                 'l.oS = l.oP + CL_PART * LQR_NT', 'l.oZ0 = l.oS + 64', 'fixed + 2LL * n * 64 > budget / 2', 'fixed + 2LL * n * ts > budget', 'l.ldn = n | 1; l.ldx = nx | 1'):
        assert term in body, term
    assert 'constexpr int CL_PART = 6;' in src and 'LQR_LDS_BYTES / 8' in body


def test_the_closed_loop_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_closed_loop_batch_host', 'tmpc_closed_loop_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 27
    assert re.search(r'^#define TMPC_CLOSED_LOOP_INFO 4$', header, re.M)
    import tunempc_amd
    assert tunempc_amd.closed_loop.closed_loop_batch is not None


def test_the_library_refuses_by_itself_what_python_refuses():
    """The entry's own checks (a caller of the C ABI does not pass through Python): TMPC_E_ARG / TMPC_E_UNSUPPORTED before any device call."""
    import ctypes as C
    from tunempc_amd._lib import load_library
    lib = load_library()
    d = (C.c_double * 8)()
    f = lib.tmpc_closed_loop_batch_host
    ok = dict(nb=1, p=2, nx=1, mb=1, nr=0, ng=0, ns=1, T=1, k0=0)
    call = lambda **kw: f(*[{**ok, **kw}[k] for k in ('nb', 'p', 'nx', 'mb', 'nr', 'ng', 'ns', 'T', 'k0')], d, d, d, d, None, None, None, None, None, None, None,
                          None, None, None, None, None, d, d)
    for kw in (dict(T=0), dict(k0=2), dict(k0=-1), dict(ns=0), dict(nr=1), dict(ng=1)):
        assert call(**kw) == -1, kw
    assert call(nx=40, mb=30) == -2 and b'nx + nu = 64' in lib.tmpc_last_error()
    from tunempc_amd import closed_loop as cl
    for nx, mb, nr in ((32, 32, 200), (24, 8, 700), (63, 1, 300)):           # the library's layout and its restatement in Python give the same size
        assert f(1, 2, nx, mb, nr, 0, 1, 1, 0, d, d, d, d, None, None, d, None, None, None, None, None, None, None, None, None, d, d) == -2
        assert re.search(r'needs (\d+) bytes', lib.tmpc_last_error().decode()).group(1) == str(cl.lds_layout(nx, mb, nr)['bytes']), (nx, mb, nr)
    none5 = [None] * 5
    assert f(1, 2, 1, 1, 0, 0, 1, 1, 0, d, d, d, d, *none5, None, None, d, None, None, None, None, d, d) == -1      # l without H
    assert b'an output without its input' in lib.tmpc_last_error()
