"""Single-precision triangular solves in the single-precision iterations (round 7; TMPC_TUNE_LOWP_TRSM, tmpc_cr.h: k_cr_trsm_dma_f32; run with -m gpu).

In the early main-phase iterations whose Schur-complement updates run in float32 (TMPC_TUNE_LOWP_SWITCH), the solves O = E L^-T that feed them now run in
float32 too.  Like the updates, this changes how the iteration gets down the central path, not the point it ends at: the Cholesky of the diagonal blocks,
the iterate and the whole centering phase stay fp64.  Checked here against the same handle with the key off (round-6 behaviour): same status, the same
iteration counts at the bench shape, Hc / P within 1e-9 of each other, Hc of both within the 1e-8 parity bar of the fp64 CPU port -- plain model at the bench
shape and at a shape with a narrow last tile, Step 1 with G, Step 2 --, the frozen-pivot fallback per problem, and a handle that alternates block widths."""
import numpy as np
import pytest
import torch  # noqa: F401

pytestmark = pytest.mark.gpu

import cpu_ipm  # noqa: E402
from tunempc_amd import synthetic  # noqa: E402

PARITY = 1e-8


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _rows(seed, nb, p, n, ng, nc):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nb, p, ng, n)); C = rng.standard_normal((nb, p, nc, n))
    ncnt = rng.integers(0, nc + 1, size=(nb, p)).astype(np.int32)
    for b in range(nb):
        for k in range(p):
            C[b, k, ncnt[b, k]:] = 0.0
    return G, C, ncnt


def _check_pair(on, off, ref, nb, same_iters, extra=()):
    assert (on['status'] == 0).all() and np.array_equal(on['status'], off['status'])
    if same_iters:
        assert np.array_equal(on['iters'], off['iters']), (on['iters'], off['iters'])
    for b in range(nb):
        for k in ('Hc', 'P') + tuple(extra):
            assert rel(on[k][b], off[k][b]) < 1e-9, (k, b, rel(on[k][b], off[k][b]))
        assert rel(on['Hc'][b], ref['Hc'][b]) < PARITY and rel(off['Hc'][b], ref['Hc'][b]) < PARITY
        assert abs(on['kappa'][b] / off['kappa'][b] - 1.0) < 1e-9


@pytest.mark.parametrize('p,nx,mb,nb', [(64, 24, 8, 4), (30, 20, 10, 3)])
def test_single_precision_solves_same_point(p, nx, mb, nb):
    from tunempc_amd._lib import HipConvexifier, FLAG_PROFILE
    A, B, H = synthetic.gen_batch(74000 + p, nb, p, nx, mb)
    ref = cpu_ipm.convexify_batch(A, B, H, threads=min(nb, 8))
    outs = {}
    for key in (1, 0):
        h = HipConvexifier(p, nx, mb, chunk=nb, flags=FLAG_PROFILE)
        h.set_tuning(lowp_trsm=key)
        h.profile()
        outs[key] = h.convexify_batch(A, B, H)
        pf = h.profile()
        h.close()
        assert pf['lowp_factorisations'] >= 3 * nb, pf          # the single-precision iterations run with the key on and off alike
    _check_pair(outs[1], outs[0], ref, nb, same_iters=(p, nx) == (64, 24))


def test_single_precision_solves_with_rows():
    """Step 1 with G and Step 2 (blocks of 144 / 160: a narrow last tile) with the key on against off, and both against cpu_ipm."""
    from tunempc_amd._lib import HipConvexifier
    p, nx, mb, nb, ng, nc = 8, 16, 4, 4, 2, 6
    n = nx + mb
    A, B, H = synthetic.gen_batch(74500, nb, p, nx, mb)
    G, C, ncnt = _rows(745, nb, p, n, ng, nc)
    J = np.concatenate([G, C], axis=2)
    r_eq = cpu_ipm.convexify_con_batch(A, B, H, G, ng=ng, threads=4)
    r_s2 = cpu_ipm.convexify_con_batch(A, B, H, J, ng=ng, ncnt=ncnt, rho=1e-2, threads=4)
    outs = {}
    for key in (1, 0):
        h = HipConvexifier(p, nx, mb, chunk=nb, ng=ng, nc=nc)
        h.set_tuning(lowp_trsm=key)
        outs[key] = (h.convexify_eq_batch(A, B, H, G), h.convexify_step2_batch(A, B, H, J, ncnt, 1e-2))
        h.close()
    _check_pair(outs[1][0], outs[0][0], r_eq, nb, same_iters=False)
    _check_pair(outs[1][1], outs[0][1], r_s2, nb, same_iters=False)


def test_single_precision_solves_frozen_pivot_fallback():
    """cond(Hhat) = 1e3 at a mid shape: where a pivot freezes under the single-precision iterations, k_ctrl_c repeats that iteration in fp64 and turns them
    off for the member; every member ends Optimal with the invariants, with the key on and off."""
    from tunempc_amd._lib import HipConvexifier
    p, nx, mb, nb = 16, 16, 4, 12
    probs = [synthetic.gen_problem(73000 + 7 * b, p, nx, mb, sigP=10.0, cond_exp=3, rad=0.9) for b in range(nb)]
    A, B, H = (np.stack([q[i] for q in probs]) for i in range(3))
    outs = []
    for key in (1, 0):
        h = HipConvexifier(p, nx, mb, chunk=nb)
        h.set_tuning(lowp_trsm=key)
        outs.append(h.convexify_batch(A, B, H))
        h.close()
    on, off = outs
    assert (on['status'] == 0).all() and (off['status'] == 0).all()
    ev = np.linalg.eigvalsh(on['Hc'])
    assert ev.min() > 0 and ((ev[:, :, -1] / ev[:, :, 0]).max(axis=1) <= on['kappa'] * (1 + 1e-7)).all()
    same = on['info'][:, 6] == off['info'][:, 6]                    # members that end at the same mu_t (a back-off may differ by one on such inputs)
    assert same.sum() >= nb // 2
    assert np.abs(on['kappa'][same] / off['kappa'][same] - 1).max() < 1e-8
    assert on['iters'].max() <= 50 + 12 * 11 + 2


def test_single_precision_solves_alternating_block_widths():
    """One handle serves Step 2 (blocks of 160), the plain model (144) and Step 1 with G (144) in turn, twice, with the float32 solves on: they write the float32
    O copies laid out by the call's block width, whose zero padding the float32 updates read -- every call agrees with cpu_ipm."""
    from tunempc_amd._lib import HipConvexifier
    p, nx, mb, nb, ng, nc = 8, 16, 4, 4, 2, 6
    n = nx + mb
    A, B, H = synthetic.gen_batch(75000, nb, p, nx, mb)
    G, C, ncnt = _rows(75, nb, p, n, ng, nc)
    J = np.concatenate([G, C], axis=2)
    r_plain = cpu_ipm.convexify_batch(A, B, H, threads=4)
    r_eq = cpu_ipm.convexify_con_batch(A, B, H, G, ng=ng, threads=4)
    r_s2 = cpu_ipm.convexify_con_batch(A, B, H, J, ng=ng, ncnt=ncnt, rho=1e-2, threads=4)
    h = HipConvexifier(p, nx, mb, chunk=nb, ng=ng, nc=nc)
    h.set_tuning(lowp_trsm=1)
    for _ in range(2):
        for out, ref in ((h.convexify_step2_batch(A, B, H, J, ncnt, 1e-2), r_s2), (h.convexify_batch(A, B, H), r_plain), (h.convexify_eq_batch(A, B, H, G), r_eq)):
            for b in range(nb):
                assert int(out['status'][b]) == int(ref['status'][b]) == 0
                assert rel(out['Hc'][b], ref['Hc'][b]) < PARITY
    h.close()
