"""CPU self-test of tests/cr_reference.py on the very inputs of tests/test_gpu_factor_kernels.py: every precision policy factors every case
without a non-positive pivot (np.linalg.cholesky / ddnum.cholesky raise on one) -- the GPU tests demand nshift == 0 on that ground -- and the
reference's own backward errors and block distances, from which the GPU tolerances are set, are printed (pytest -s) and sanity-checked against
the unit roundoff of the policy's number format."""
import numpy as np
import pytest

import cr_reference as cr

U64, U32, UDD = 2.0 ** -53, 2.0 ** -24, 2.0 ** -104


def _sched(p):
    from tunempc_amd._lib import cr_schedule
    return cr_schedule(p)


def test_generator_hits_the_condition_number():
    for (p, d, cond) in cr.F32_CASES + cr.FP64_CASES + cr.DD_CASES + cr.LIST_CASES:
        got = cr.case(p, d, cond)['cond'][0]
        print(f'p {p:2d} d {d:3d} target {cond:.0e} cond(T) {got:.2e}')
        assert cond / 4 <= got <= cond * 4


@pytest.mark.parametrize('p,d,cond', sorted(set(cr.F32_CASES + cr.FP64_CASES)))
def test_policies_factor_and_solve(p, d, cond):
    c = cr.case(p, d, cond)
    D, Cc, b = c['D'][0], c['Cc'][0], c['b3'][0]
    Tl = cr.dense(D, Cc, np.longdouble)
    sched = _sched(p)
    policies = cr.POLICIES if (p, d, cond) in cr.F32_CASES else ('fp64',)
    refs = {pol: cr.reference(sched, D, Cc, b, pol) for pol in policies}       # (LinAlgError = a non-positive pivot = failure)
    xt = cr.solve_truth(Tl, b.reshape(p * d, 3))
    for pol, r in refs.items():
        be = max(cr.backward_error(Tl, r['x'][..., q], b[..., q], c['norm2'][0]) for q in range(3))
        fe = max(cr.rel(r['x'][..., q].ravel(), xt[:, q].astype(np.float64)) for q in range(3))
        dl = max(cr.rel(r['L'][i], refs['fp64']['L'][i]) for i in range(p))
        print(f'p {p:2d} d {d:3d} cond {c["cond"][0]:.2e} {pol:12s} backward {be:.2e} forward {fe:.2e} max dist(L, fp64 L) {dl:.2e}')
        u = U64 if pol == 'fp64' else U32
        assert be < 4 * u                                 # a reference that is itself off by more than a few roundoffs of its format is no yardstick
        assert fe < c['cond'][0] * 4 * u
        assert r['top'] < 2 * p


def test_list_case_batches_factor_in_every_policy():
    for (p, d, cond) in cr.LIST_CASES:
        c = cr.case(p, d, cond, nb=6)
        for b in range(6):
            for pol in cr.POLICIES:
                cr.reference(_sched(p), c['D'][b], c['Cc'][b], c['b1'][b], pol)


@pytest.mark.parametrize('p,d,cond', cr.DD_CASES)
def test_dd_reference(p, d, cond):
    c = cr.case(p, d, cond)
    D, Cc, b = c['D'][0], c['Cc'][0], c['b1'][0]
    cr.reference(_sched(p), D, Cc, b, 'fp64')             # (the fp64 Cholesky gets through: so does the dd one)
    r = cr.reference_dd(_sched(p), D, Cc, b)
    res = cr.dd_residual(D, Cc, r['xh'], r['xl'], b)
    nT = c['norm2'][0]
    q = np.linalg.norm(res) / (nT * np.linalg.norm(r['xh']))
    q64 = np.linalg.norm(cr.dd_residual(D, Cc, r['xh'], np.zeros_like(r['xl']), b)) / (nT * np.linalg.norm(r['xh']))
    print(f'p {p} d {d:3d} cond {c["cond"][0]:.2e} dd residual {q:.2e}; without the low words {q64:.2e}')
    assert q < UDD and q64 > 1e6 * q                      # the measure itself tells a dd solution from its high words


def test_dd_residual_against_mpmath():
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 60
    for (p, d) in [(1, 4), (2, 3), (3, 4)]:
        rng = np.random.default_rng(p)
        D, Cc, _ = cr.spd_cyclic(rng, p, d)
        xh = rng.standard_normal((p, d)); xl = xh * 2.0 ** -54 * rng.standard_normal((p, d)); b = rng.standard_normal((p, d))
        r = cr.dd_residual(D, Cc, xh, xl, b)
        Tm = mp.zeros(p * d)
        for k in range(p):
            kn = (k + 1) % p
            for i in range(d):
                for j in range(d):
                    Tm[k * d + i, k * d + j] += mp.mpf(float(D[k, i, j]))
                    Tm[k * d + i, kn * d + j] += mp.mpf(float(Cc[k, i, j])); Tm[kn * d + j, k * d + i] += mp.mpf(float(Cc[k, i, j]))
        xm = mp.matrix([mp.mpf(float(a)) + mp.mpf(float(c_)) for a, c_ in zip(xh.ravel(), xl.ravel())])
        rm = mp.matrix([mp.mpf(float(v)) for v in b.ravel()]) - Tm * xm
        assert all(abs(mp.mpf(float(r.ravel()[i])) - rm[i]) <= 2.0 ** -52 * abs(rm[i]) for i in range(p * d))      # every row correctly rounded
