"""CPU tests of the finite-horizon LQR pass: the numpy statement tests/lqr_horizon_reference.py against itself (the stage recursion (a) against the dense
horizon KKT solve (b)), the counts, the certificate with and without the shift of the terminal weight, the long-horizon limit, the figures of the AWE golden
that bound the GPU test, and the host-side argument checks of tunempc_amd.lqr.horizon_* (no device needed).

Measured with numpy on the synthetic cases (gen_problem seed 7, P default_rng(5)): (a) vs (b) <= 3.0e-12 of max(1, max|K_0|) (bench stage shape, terminal
constraint, N = 8), dK0 <= 5.4e-13; without the shift dK0 = 9.6, 0.36, 2.1e-3, 1.6e-5 at N = 1, 2, 5, 8; at N = 24 K_0 equals the periodic gain to 2.2e-16
(rho = 0.078).  AWE golden (tests/golden/awe_step2_n15.npz: p 40, nx 9, nu 6, 3 + 0..4 rows), terminal='cost', N = 20, all 40 phases, per phase and relative
to max(1, max|K_0| of the phase): (a) vs (b) up to 4.6e-10 (H side; 2.5e-10 on the Hc side), dK0_rel up to 6.4e-10 (phase 28); relative to the largest gain
of all phases, max|K_0| = 37.7, they are 2.6e-11 and 3.6e-11.  c_0 is 0, 1 or 2, equal on both sides."""
import os
import re

import numpy as np
import pytest

import lqr_ctg_reference as lc
import lqr_horizon_reference as lh
from test_lqr_ctg_cpu import load_awe

# measured on the AWE golden by the numpy reference alone (see the module docstring); test_gpu_horizon_lqr.py takes its bound for this golden from them
AWE_H_AB_DISAGREEMENT = 4.7e-10      # max over the 40 phases and both sides of |u_0 (b) + K_0 x_0 (a)| / max(1, max|K_0|)
AWE_H_DK = 6.4e-10                   # max over the 40 phases of max|K_0(H) - K_0(Hc)| / max(1, max|K_0(Hc)|)
AWE_H_BOUND = 10.0 * max(AWE_H_AB_DISAGREEMENT, AWE_H_DK)      # what the GPU test allows against the reference and for dK0_rel: 6.4e-9
NOISE_MARGIN = 1.5                   # the figures are rounding noise: another BLAS build may move them, not by more than this
AB_BOUND = 1e-10                     # (a) vs (b) on the small cases, relative to max(1, max|K_0|): about 30 x the worst value measured (3e-12)

# (case, terminal, horizons): every synthetic case in the modes where it is feasible
SMALL = [(lh.case_no_rows, 'constraint', (1, 2, 3, 4, 7)), (lh.case_ragged_rows, 'constraint', (1, 2, 3, 4, 5, 8)),
         (lh.case_bench_stage_shape, 'constraint', (1, 8, 9)), (lh.case_ragged_rows, 'cost', (1, 2, 5, 8)),
         (lh.case_bench_stage_shape_ragged, 'cost', (1, 3, 9)), (lh.case_single_phase, 'constraint', (1, 2, 5)), (lh.case_single_phase, 'cost', (1, 2, 5)),
         (lh.case_no_feasible_subspace, 'cost', (1,))]
IDS = ['%s-%s' % (f.__name__, t) for f, t, _ in SMALL]


def both_sides(c, N, terminal, shift=True, b=0):
    """The passes of all phases on the H side (terminal weight P when shift) and on the Hc side of member b -> (resH, resC)."""
    J = None if c['J'] is None else c['J'][b]
    return (lh.horizon_lqr_phases(c['A'][b], c['B'][b], c['H'][b], J, c['rows'][b], N, terminal, c['P'][b] if shift else None),
            lh.horizon_lqr_phases(c['A'][b], c['B'][b], c['Hc'][b], J, c['rows'][b], N, terminal, None))


@pytest.mark.parametrize('case,terminal,horizons', SMALL, ids=IDS)
def test_recursion_against_the_dense_horizon_kkt_solve_and_the_certificate(case, terminal, horizons):
    c = case()
    J = None if c['J'] is None else c['J'][0]
    for N in horizons:
        rH, rC = both_sides(c, N, terminal)
        assert not any(r['infeasible'] for r in rH + rC)
        ab = max(lh.ab_disagreement(c['A'][0], c['B'][0], c[s][0], J, c['rows'][0], N, terminal, Pf, r).max()
                 for s, Pf, r in (('H', c['P'][0], rH), ('Hc', None, rC)))
        dK = max(np.abs(h['K0'] - k['K0']).max() for h, k in zip(rH, rC))
        sd = max(np.abs(h['Pz0'] - k['Pz0']).max() for h, k in zip(rH, rC))
        feas = max(r['feas'] / max(1.0, np.abs(r['K']).max()) for r in rH + rC)
        print(case.__name__, terminal, 'N', N, 'c_0', [int(r['cnt'][0]) for r in rC], 'a vs b %.1e  dK0 %.1e  subspaces %.1e  feas %.1e' % (ab, dK, sd, feas))
        assert ab <= AB_BOUND, (N, ab)
        assert dK <= 1e-10 and sd <= 1e-12 and feas <= 1e-10, (N, dK, sd, feas)
        assert all((h['cnt'] == k['cnt']).all() for h, k in zip(rH, rC))


def test_expected_counts():
    cnt = lambda f, N, term, k0=0: lh.horizon_lqr(f()['A'][0], f()['B'][0], f()['Hc'][0], None if f()['J'] is None else f()['J'][0], f()['rows'][0], N, k0,
                                                  term)['cnt'].tolist()
    for k0 in range(3):                                                    # no rows, one input: x_N = 0 costs one state dimension per stage
        assert [cnt(lh.case_no_rows, N, 'constraint', k0)[0] for N in (1, 2, 3, 4, 7)] == [2, 1, 0, 0, 0]
        assert cnt(lh.case_no_rows, 7, 'constraint', k0) == [0, 0, 0, 0, 0, 1, 2]
    for k0 in range(2):                                                    # 8 inputs, 5 rows: three free inputs per stage
        assert [cnt(lh.case_bench_stage_shape, N, 'constraint', k0)[0] for N in (1, 8, 9)] == [21, 0, 0]
        assert cnt(lh.case_bench_stage_shape, 9, 'constraint', k0) == [0, 0, 3, 6, 9, 12, 15, 18, 21]
    assert cnt(lh.case_ragged_rows, 4, 'constraint') == [0, 0, 1, 2] and cnt(lh.case_ragged_rows, 8, 'cost') == [0] * 8
    assert cnt(lh.case_no_feasible_subspace, 1, 'cost') == [1]


def test_without_the_shift_the_gains_differ():
    """The contrast: both sides with a zero terminal weight are different problems, by O(1) at short horizons; the difference fades with N."""
    c = lh.case_ragged_rows()
    d = {}
    for N in (1, 2, 5, 8):
        rH, rC = both_sides(c, N, 'cost', shift=False)
        d[N] = max(np.abs(h['K0'] - k['K0']).max() for h, k in zip(rH, rC))
    print(d)
    assert d[1] >= 1e-2 and d[2] >= 1e-2 and d[8] < d[5] < d[2] < d[1]


@pytest.mark.parametrize('N', [4, 7])
def test_no_feasible_subspace(N):
    c = lh.case_no_feasible_subspace()
    for s in ('H', 'Hc'):
        res = lh.horizon_lqr_phases(c['A'][0], c['B'][0], c[s][0], c['J'][0], c['rows'][0], N, 'cost', None)
        assert all(r['infeasible'] and r['stage'] == N - 4 for r in res)           # three rows on two inputs: one dimension per stage, nx = 4
    c = lh.case_bench_stage_shape()                                                # r_k >= nu at every stage under a terminal constraint: the same end
    J = np.concatenate([c['J'][0], np.random.default_rng(1).standard_normal((2, 3, 32))], axis=1)
    assert lh.horizon_lqr(c['A'][0], c['B'][0], c['Hc'][0], J, None, 2, 0, 'constraint')['infeasible']                # (at its first stage: 32 generic rows leave nothing of x)


def test_a_long_horizon_gives_the_periodic_gain():
    c = lh.case_ragged_rows()
    per = lc.periodic_lqr(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], tol=1e-14)
    res = lh.horizon_lqr_phases(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], 24, 'constraint')
    d = max(np.abs(res[k]['K0'] - per['K'][k]).max() for k in range(3))
    d6 = max(np.abs(r['K0'] - per['K'][k]).max() for k, r in enumerate(lh.horizon_lqr_phases(c['A'][0], c['B'][0], c['Hc'][0], c['J'][0], c['rows'][0], 6)))
    print('rho %.3f  N = 24: %.1e  N = 6: %.1e' % (per['rho'], d, d6))
    assert per['converged'] and not per['cnt'].any() and d <= 1e-12
    assert d6 >= 1e-6                                                      # at the horizons people use they are different numbers


def test_awe_golden_figures_that_bound_the_gpu_test():
    d = load_awe()
    A, B, J, rows = d['A'][0], d['B'][0], d['J'][0], d['ng'] + d['ncnt'][0]
    rH = lh.horizon_lqr_phases(A, B, d['H'][0], J, rows, 20, 'cost', d['P'][0]); rC = lh.horizon_lqr_phases(A, B, d['Hc'][0], J, rows, 20, 'cost', None)
    assert not any(r['infeasible'] for r in rH + rC)
    ab = max(lh.ab_disagreement(A, B, d['H'][0], J, rows, 20, 'cost', d['P'][0], rH).max(), lh.ab_disagreement(A, B, d['Hc'][0], J, rows, 20, 'cost', None, rC).max())
    dk = lh.dk0_rel(rH, rC)
    c0 = [int(r['cnt'][0]) for r in rC]
    print('a vs b %.2e  dK0_rel %.2e (phase %d)  max|K_0| %.1f  c_0 %s  feas %.1e' % (ab, dk.max(), dk.argmax(), max(np.abs(r['K0']).max() for r in rC), c0,
                                                                                 max(r['feas'] for r in rH + rC)))
    assert c0 == [int(r['cnt'][0]) for r in rH] and set(c0) == {0, 1, 2} and max(np.abs(h['Pz0'] - k['Pz0']).max() for h, k in zip(rH, rC)) <= 1e-12
    assert ab <= NOISE_MARGIN * AWE_H_AB_DISAGREEMENT and dk.max() <= NOISE_MARGIN * AWE_H_DK, (ab, dk.max())
    assert max(r['feas'] for r in rH + rC) <= 1e-10


# ----------------------------------------------------------------------------- the C ABI and the host-side argument checks (no device needed)
def test_the_horizon_entries_are_declared_exported_and_bound():
    from tunempc_amd._lib import EXPORTS, load_library
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    header = open(os.path.join(root, 'include', 'tunempc_hip.h')).read()
    lib = load_library()
    for name in ('tmpc_horizon_lqr_batch_host', 'tmpc_horizon_lqr_batch_device'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 24


def _batch(nb=2, p=3, nx=4, mb=2):
    return np.zeros((nb, p, nx, nx)), np.zeros((nb, p, nx, mb)), np.tile(np.eye(nx + mb), (nb, p, 1, 1))


def test_argument_checks_before_any_device_call():
    from tunempc_amd import lqr
    A, B, H = _batch()
    for bad in (0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match='horizon must be an int >= 1'):
            lqr.horizon_lqr_batch(A, B, H, bad)
    for bad in ([3], [0, -1], [], [0.5], [[0, 1]]):
        with pytest.raises(ValueError, match='phases must'):
            lqr.horizon_lqr_batch(A, B, H, 4, phases=bad)
    for bad in ('none', 'Constraint', None, 1):
        with pytest.raises(ValueError, match="terminal must be 'constraint' \\(x_N = 0\\) or 'cost'"):
            lqr.horizon_lqr_batch(A, B, H, 4, terminal=bad)
    with pytest.raises(ValueError, match="terminal='cost' needs P"):
        lqr.horizon_equivalence_batch(A, B, H, H, 4, terminal='cost')
    with pytest.raises(ValueError, match='horizon_lqr_batch: ncnt / ng describe the rows of J, which is None'):
        lqr.horizon_lqr_batch(A, B, H, 4, ng=1)
    with pytest.raises(ValueError, match='horizon_lqr_batch: Pf .* expected'):
        lqr.horizon_lqr_batch(A, B, H, 4, Pf=np.zeros((2, 3, 4, 3)))
    with pytest.raises(ValueError, match='0 < rank_tol < 1 expected'):
        lqr.horizon_lqr_batch(A, B, H, 4, rank_tol=0.0)
    args = (np.eye(2), np.ones((2, 1)), np.eye(2), np.eye(1), np.zeros((2, 1)))
    with pytest.raises(ValueError, match='horizon must be an int >= 1'):
        lqr.horizon_lqr(*args, 0)
    with pytest.raises(ValueError, match="terminal='cost' needs P"):
        lqr.horizon_equivalence(*args, [np.zeros((3, 3))], 3, terminal='cost')
    with pytest.raises(ValueError, match='Pf must be one \\(nx, nx\\) matrix or a list of p = 1 of them'):
        lqr.horizon_lqr(*args, 3, Pf=np.eye(3))


def test_mixed_numpy_and_torch_arguments_are_refused():
    import torch
    from tunempc_amd import lqr
    A, B, H = _batch()
    with pytest.raises(ValueError, match='horizon_lqr_batch: A, B, H .* must be all numpy arrays or all torch tensors'):
        lqr.horizon_lqr_batch(A, torch.zeros(B.shape, dtype=torch.float64), H, 4)
    with pytest.raises(ValueError, match='horizon_equivalence_batch: A, B, H .* must be all numpy arrays or all torch tensors \\(Hc differs\\)'):
        lqr.horizon_equivalence_batch(A, B, H, torch.zeros(H.shape, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match='J must be a numpy array like A, B, H'):
        lqr.horizon_lqr_batch(A, B, H, 4, J=torch.zeros((2, 3, 1, 6), dtype=torch.float64))


def test_refusals_carry_the_library_message():
    """A shape beyond the 160 KB LDS layout, and what the library checks by itself, are refused before it touches a device."""
    from tunempc_amd import lqr
    A, B, H = _batch(1, 2, 32, 32)
    with pytest.raises(NotImplementedError, match='nx = 32, nu = 32 with room for 40 rows per stage and a constraint-to-go needs \\d+ bytes of LDS \\(limit 163840\\)'):
        lqr.horizon_lqr_batch(A, B, H, 3, J=np.zeros((1, 2, 40, 64)))
    with pytest.raises(NotImplementedError, match='stage blocks up to nx \\+ nu = 64'):
        lqr.horizon_lqr_batch(*_batch(1, 2, 40, 30), 3)
    A, B, H = _batch()
    with pytest.raises(ValueError, match='0 <= ng <= nr, the row capacity per stage.*ng = 3, nr = 2'):
        lqr.horizon_lqr_batch(A, B, H, 3, J=np.zeros((2, 3, 2, 6)), ng=3)


def test_the_layout_is_valid_without_rows():
    """lqr_ctg_lds(nx, mb, nr = 0) restated: the border holds min(mb, nx) rows, the stack max(nx, mb) rows (the constraint-to-go alone, up to the nx rows of a
    terminal constraint), every buffer is non-empty, and the bench stage shape fits."""
    def layout(nx, mb, nr):
        n = nx + mb
        nbd, ms = min(mb, nr + nx), max(nr + nx, mb)
        ld, ldp, ldc = (n + nbd) | 1, nx | 1, n | 1
        sizes = dict(E=nx * ld, P=nx * ldp, W=max(nx, mb + nbd) * ld, Hb=(n + nbd) * ld, C0=ms * ldc, C1=ms * ldc, N0=nx * ldp, N1=nx * ldp, red=16)
        return nbd, ms, sizes
    for nx, mb in ((1, 1), (3, 1), (3, 2), (4, 2), (24, 8), (9, 6), (2, 30), (20, 12)):
        nbd, ms, sizes = layout(nx, mb, 0)
        assert nbd == min(mb, nx) and ms >= nx and ms >= mb and min(sizes.values()) > 0
        assert sizes['W'] >= (mb + nbd) * ((nx + mb + nbd) | 1)             # the second buffer of the solve, rho = nbd
        assert 8 * sum(sizes.values()) <= 160 * 1024
    assert 8 * sum(layout(24, 8, 0)[2].values()) < 8 * sum(layout(24, 8, 5)[2].values()) < 61344
