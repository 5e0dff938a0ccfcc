"""tests/phi_reference.py against the definition of the model, against the CPU oracle's path, and against mutated copies of itself (no device).

The GPU test (tests/test_gpu_phi_kernels.py) compares the multiplier kernels of tunempc_amd/csrc/tmpc_phi.h with this reference.  Here the reference is tied to
something that shares no formula with it: the HKM Schur matrix of the whole rows model built by brute force -- the constraint operator applied to every unit vector
of (svec P, tau, alpha, phi, t) and T_ij = sum_cones <A_i, sym(X A_j S^-1)> -- and the Newton step of a dense solve of that matrix (a, b).  The cases of the GPU
test are solved on the oracle (c).  Each numerical mutation of profiles/phi_kernel_mutations.txt, applied to the reference, breaks (a) or (b) (d)."""
import numpy as np
import pytest

import convexify_oracle as co
import phi_kernel_cases as pc
import phi_reference as ph
import schur_reference as sr

LD = np.longdouble
EPS = sr.EPS


# ---------------------------------------------------------------------------------------------------------------- a random interior point of the rows model
def _spd(rng, n, lo=0.3):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return co.symmetrize((Q * rng.uniform(lo, 2.0, n)) @ Q.T)


def _model(seed, p, nx, mb, rows, norm, rho=0.3):
    """rows: rows of [G_k; C_k] per stage; norm: per stage the arrow blocks [(a0, m)].  Everything a cone of the model holds, at a random interior point."""
    rng = np.random.default_rng(seed)
    n = nx + mb
    g = dict(p=p, nx=nx, n=n, d=nx * (nx + 1) // 2, rows=rows, norm=norm, wr=rho * 1.7)
    g['V'] = rng.standard_normal((p, nx, n)) / np.sqrt(nx)
    g['Hb'] = np.stack([co.symmetrize(rng.standard_normal((n, n))) for _ in range(p)])
    g['X'] = np.stack([[_spd(rng, n) for _ in range(p)] for _ in range(2)])          # [2, p, n, n]
    g['S'] = np.stack([[_spd(rng, n) for _ in range(p)] for _ in range(2)])
    g['Rd'] = 0.1 * np.stack([[co.symmetrize(rng.standard_normal((n, n))) for _ in range(p)] for _ in range(2)])
    g['x0'], g['s0'], g['rd0'] = 0.21, 0.37, 0.013
    g['G'] = [rng.standard_normal((rows[k], n)) for k in range(p)]
    g['phi'] = [rng.uniform(0.2, 1.5, rows[k]) for k in range(p)]
    g['z'] = [rng.uniform(0.2, 1.5, rows[k]) for k in range(p)]
    g['t'] = [[float(np.linalg.norm(g['wr'] * g['phi'][k][a0:a0 + m]) + rng.uniform(0.3, 1.0)) for a0, m in norm[k]] for k in range(p)]
    g['Xa'] = [[_spd(rng, m + 1) for a0, m in norm[k]] for k in range(p)]
    return g


class Brute:
    """the model as a list of cones (X_c, S_c, Rd_c) and of variables with their images A_j[c] in every cone and their cost c_j -- nothing stage-local about it"""

    def __init__(self, g):
        p, nx, n, d = g['p'], g['nx'], g['n'], g['d']
        self.g = g
        L = lambda M: np.asarray(M, LD)
        self.X, self.S, self.Rd, self.cone = [], [], [], {}

        def add(key, X, S, Rd=None):
            self.cone[key] = len(self.X)
            self.X.append(L(X)); self.S.append(L(S)); self.Rd.append(np.zeros_like(L(S)) if Rd is None else L(Rd))
        for k in range(p):
            for r in (0, 1):
                add(('lmi', r, k), g['X'][r, k], g['S'][r, k], g['Rd'][r, k])
        add(('s0',), [[g['x0']]], [[g['s0']]], [[g['rd0']]])
        for k in range(p):
            for i in range(g['rows'][k]):
                add(('lin', k, i), [[g['z'][k][i]]], [[g['phi'][k][i]]])
            for e, (a0, m) in enumerate(g['norm'][k]):
                add(('arrow', k, e), g['Xa'][k][e], ph.arrow(g['t'][k][e], g['phi'][k][a0:a0 + m], g['wr']))
        self.Si = [ph.inverse(S) for S in self.S]
        self.var, self.A, self.cost = {}, [], []

        def new(key, cost=0):
            self.var[key] = len(self.A)
            self.A.append({}); self.cost.append(LD(cost))
            return self.A[-1]
        ia, ib = sr.tri_idx(nx)
        for j in range(p):
            for idx in range(d):
                E = np.zeros((p, nx, nx), LD); E[j, ia[idx], ib[idx]] = 1; E[j, ib[idx], ia[idx]] = 1
                dM = sr._calH(L(g['V']), E, nx, -1)
                A = new(('P', j, idx))
                for k in range(p):
                    if dM[k].any():
                        A[self.cone['lmi', 0, k]] = dM[k]; A[self.cone['lmi', 1, k]] = -dM[k]
        A = new(('tau',), 1)
        for k in range(p):
            A[self.cone['lmi', 1, k]] = np.eye(n, dtype=LD)
        A = new(('alpha',))
        for k in range(p):
            A[self.cone['lmi', 0, k]] = L(g['Hb'][k]); A[self.cone['lmi', 1, k]] = -L(g['Hb'][k])
        A[self.cone['s0',]] = np.ones((1, 1), LD)
        for k in range(p):
            for i in range(g['rows'][k]):
                gg = np.outer(L(g['G'][k][i]), L(g['G'][k][i]))
                A = new(('phi', k, i))
                A[self.cone['lmi', 0, k]] = gg; A[self.cone['lmi', 1, k]] = -gg; A[self.cone['lin', k, i]] = np.ones((1, 1), LD)
                for e, (a0, m) in enumerate(g['norm'][k]):
                    if a0 <= i < a0 + m:
                        A[self.cone['arrow', k, e]] = ph._E(i - a0, m, g['wr'], LD)
            for e, (a0, m) in enumerate(g['norm'][k]):
                new(('t', k, e), 1)[self.cone['arrow', k, e]] = np.eye(m + 1, dtype=LD)
        nv = len(self.A)
        self.T = np.zeros((nv, nv), LD)
        for j in range(nv):
            F = {c: sr._sym(self.X[c] @ Aj @ self.Si[c]) for c, Aj in self.A[j].items()}
            for i in range(nv):
                self.T[i, j] = sum(np.sum(Ai * F[c]) for c, Ai in self.A[i].items() if c in F)

    def adjoint(self, Y):
        """sum_cones <A_j, Y_c> per variable"""
        return np.array([sum(np.sum(Aj * Y[c]) for c, Aj in A.items()) for A in self.A], LD)

    def primal_residual(self, X=None):
        return np.asarray(self.cost, LD) - self.adjoint(self.X if X is None else X)

    def newton(self, sig, corr=None):
        """dense solve: -> dy, dS_c, dX_c per cone"""
        Tc = [LD(sig) * self.Si[c] - sr._sym(self.X[c] @ self.Rd[c] @ self.Si[c]) - (0 if corr is None else corr[c]) for c in range(len(self.X))]
        rhs = self.adjoint(Tc) - np.asarray(self.cost, LD)
        dy = np.asarray(np.linalg.solve(np.asarray(self.T, float), np.asarray(rhs, float)), LD)
        dy = dy + np.asarray(np.linalg.solve(np.asarray(self.T, float), np.asarray(rhs - self.T @ dy, float)), LD)       # one refinement step in extended precision
        dS = [self.Rd[c].copy() for c in range(len(self.X))]
        for j, A in enumerate(self.A):
            for c, Aj in A.items():
                dS[c] = dS[c] + dy[j] * Aj
        dX = [LD(sig) * self.Si[c] - self.X[c] - sr._sym(self.X[c] @ dS[c] @ self.Si[c]) - (0 if corr is None else corr[c]) for c in range(len(self.X))]
        return dy, dS, dX, rhs


MODELS = [
    dict(seed=1, p=2, nx=3, mb=1, rows=[1, 1], norm=[[], []]),                          # Step 1 with G at p = 2
    dict(seed=2, p=1, nx=3, mb=1, rows=[2], norm=[[]]),                                 # p = 1: a + b
    dict(seed=3, p=3, nx=2, mb=2, rows=[3, 1, 2], norm=[[(0, 1), (1, 2)], [(0, 1)], [(0, 1), (1, 1)]]),      # ng = 1, ragged rows of C, two arrow blocks
    dict(seed=4, p=2, nx=2, mb=1, rows=[2, 0], norm=[[(0, 2)], []]),                    # ng = 0: one arrow block at a0 = 0, a stage without rows
]
MUTATIONS = ('c_tau_sign', 'gsg_other_cone', 'arrow_residual_factor', 'a_b_swapped', 'corrp_dropped', 'acor_without_inverse', 'ap_ad_swapped')


def _stage(g, k, mut=None):
    arrows = [(a0, m, g['t'][k][e], g['Xa'][k][e]) for e, (a0, m) in enumerate(g['norm'][k])]
    Si = np.stack([ph.inverse(g['S'][r, k]) for r in (0, 1)])
    return ph.stage_system(g['X'][:, k], Si, g['V'][k], g['Hb'][k], g['G'][k], g['phi'][k], g['z'][k], g['nx'], arrows, g['wr'], mut=mut)


def _local_vars(bm, g, k):
    return [bm.var['phi', k, i] for i in range(g['rows'][k])] + [bm.var['t', k, e] for e in range(len(g['norm'][k]))]


def schur_mismatch(g, bm, mut=None):
    """largest |structured piece - brute-force entry| over T_loc,loc, a, b (a + b at p = 1), c_tau, c_alpha, the arrow entries and the stationarity residuals,
    relative to the largest entry of the brute-force matrix"""
    p, d = g['p'], g['d']
    worst = LD(0)
    res = bm.primal_residual()
    for k in range(p):
        s = _stage(g, k, mut)
        lv = _local_vars(bm, g, k)
        if not lv:
            continue
        kn = (k + 1) % p
        m = g['rows'][k]
        pk = [bm.var['P', k, i] for i in range(d)]; pkn = [bm.var['P', kn, i] for i in range(d)]
        diffs = [s['T'] - bm.T[np.ix_(lv, lv)], s['c_tau'] - bm.T[lv, bm.var['tau',]], s['c_alpha'] - bm.T[lv, bm.var['alpha',]], s['res'] - res[lv]]
        if p == 1:
            diffs.append(s['a'] + s['b'] - bm.T[np.ix_(lv[:m], pk)])
        else:
            diffs += [s['a'] - bm.T[np.ix_(lv[:m], pk)], s['b'] - bm.T[np.ix_(lv[:m], pkn)]]
            others = [bm.var['P', j, i] for j in range(p) if j not in (k, kn) for i in range(d)]
            assert not bm.T[np.ix_(lv, others)].any()              # the stage-local rows reach P_k and P_k+1 only
        assert not bm.T[np.ix_(lv[m:], pk + pkn)].any()            # the epigraph variables do not reach P
        worst = max([worst] + [np.abs(x).max() for x in diffs if x.size])
    return float(worst / np.abs(bm.T).max())


# Both sides evaluate the same bilinear forms in np.longdouble (2^-64) with at most 4 n + 12 nested operations per entry; the brute-force sum over the cones cancels
# at most by the condition of X S^-1 (< 50 for these spectra, 0.3 .. 2).  (4 n + 12) * 50 * 2^-64 < EPS = 2^-53 for every n here; 8 EPS leaves three bits of margin.
# A mutation changes an entry by its own size (a sign, a factor 2, another cone): twelve orders above.
TOL = 8 * EPS


@pytest.mark.parametrize('mdl', MODELS, ids=lambda m: f"seed{m['seed']}-p{m['p']}")
def test_structured_pieces_equal_the_brute_force_schur_matrix(mdl):
    """(a) T_loc,loc with z / phi on its diagonal, a, b, c_tau, c_alpha, the arrow entries T[phi_a, phi_q], T[phi_q, t], T[t, t], and the stationarity residuals
    (-2 w X[0, q+1], 1 - tr X among them) equal the entries of the matrix built from the constraint operator alone; the matrix is symmetric positive definite"""
    g = _model(**mdl)
    bm = Brute(g)
    assert np.abs(bm.T - bm.T.T).max() <= TOL * np.abs(bm.T).max()
    assert np.linalg.eigvalsh(np.asarray(bm.T, float)).min() > 0
    assert schur_mismatch(g, bm) <= TOL


def newton_mismatch(g, bm, mut=None):
    """(b) with the Newton step of the dense solve: largest relative mismatch of the reference's right-hand sides, dz, arrow dX, Mehrotra terms and update against
    the brute-force cones, predictor (sig = 0) then corrector (sig > 0 with the predictor's second-order terms)"""
    p = g['p']
    worst = LD(0)
    rel = lambda a, b: np.abs(np.asarray(a, LD) - b).max() / max(np.abs(b).max(), LD(1e-300)) if np.size(b) else LD(0)
    dy1, dS1, dX1, rhs1 = bm.newton(0.0)
    # the step satisfies the linearised equations: primal feasibility after the full step, linear in X
    full = [bm.X[c] + dX1[c] for c in range(len(bm.X))]
    assert np.abs(bm.primal_residual(full)).max() <= 1e3 * EPS * max(1.0, float(np.abs(rhs1).max()))
    corr = [sr._sym(dX1[c] @ dS1[c] @ bm.Si[c]) for c in range(len(bm.X))]
    # the second-order term is what the linearisation leaves of the complementarity product: sym((X + dX)(S + dS) S^-1) = sig S^-1 + corr
    for c in range(len(bm.X)):
        assert np.abs(sr._sym((bm.X[c] + dX1[c]) @ (bm.S[c] + dS1[c]) @ bm.Si[c]) - corr[c]).max() <= 1e3 * EPS * max(1.0, float(np.abs(corr[c]).max()))
    sig = 0.05
    dy2, dS2, dX2, rhs2 = bm.newton(sig, corr)
    ap, ad = 0.7, 0.4
    for pas, (dy, dS, dX, rhs, sg) in enumerate(((dy1, dS1, dX1, rhs1, 0.0), (dy2, dS2, dX2, rhs2, sig)), 1):
        for k in range(p):
            m = g['rows'][k]
            lv = _local_vars(bm, g, k)
            if not lv:
                continue
            T1, T2 = (sg * bm.Si[c] - sr._sym(bm.X[c] @ bm.Rd[c] @ bm.Si[c]) - (corr[c] if pas == 2 else 0) for c in (bm.cone['lmi', 0, k], bm.cone['lmi', 1, k]))
            lin = [bm.cone['lin', k, i] for i in range(m)]
            corrp = np.array([corr[c][0, 0] for c in lin], LD)
            if m:                                                  # pass 1 wrote corrp = dz dphi / phi
                worst = max(worst, rel(ph.mehrotra_rows([dX1[c][0, 0] for c in lin], [dS1[c][0, 0] for c in lin], g['phi'][k])[0], corrp))
            r = ph.rhs_rows(T1, T2, g['G'][k], g['phi'][k], sg, corrp if (pas == 2 and mut != 'corrp_dropped') else None)[0]
            r = np.concatenate([r, np.zeros(len(lv) - m, LD)])
            dphi = dy[lv[:m]]
            dz = ph.dual_direction(g['phi'][k], g['z'][k], dphi, sg, corrp if pas == 2 else None)[0]
            if m:
                worst = max(worst, rel(dz, np.array([dX[c][0, 0] for c in lin], LD)))
            for e, (a0, am) in enumerate(g['norm'][k]):
                c = bm.cone['arrow', k, e]
                cor = corr[c] if pas == 2 else None
                rq, rt = ph.arrow_rhs(bm.Si[c], sg, g['wr'], cor)[:2]
                r[a0:a0 + am] += rq; r[m + e] = rt
                dSa = ph.arrow(dy[bm.var['t', k, e]], dphi[a0:a0 + am], g['wr'])
                worst = max(worst, rel(dSa, dS[c]), rel(ph.arrow_dX(bm.X[c], bm.Si[c], dSa, sg, cor)[0], dX[c]))
                if pas == 1:
                    ac = ph.arrow_corrector(dX[c], dSa, bm.Si[c])[0] if mut != 'acor_without_inverse' else sr._sym(dX[c] @ dSa)
                    worst = max(worst, rel(ac, corr[c]))
                else:
                    # the update: S is linear in (t, phi), which move by ad; X moves by ap and the primal residual of t shrinks by 1 - ap
                    a_phi, a_z = (ap, ad) if mut == 'ap_ad_swapped' else (ad, ap)
                    phin = ph.update(g['phi'][k][a0:a0 + am], dphi[a0:a0 + am], a_phi)[0]
                    tn = ph.update(g['t'][k][e], dy[bm.var['t', k, e]], a_phi)[0]
                    worst = max(worst, rel(ph.arrow(tn, phin, g['wr']), bm.S[c] + ad * dS[c]))
                    Xn = ph.update(bm.X[c], dX[c], a_z, symmetric=True)[0]
                    rt0 = ph.arrow_residual(bm.X[c], g['wr'])[1]; rt1 = ph.arrow_residual(Xn, g['wr'])[1]
                    worst = max(worst, abs(rt1 - (1 - ap) * rt0) / max(abs(rt0), LD(1e-3)))
            worst = max(worst, rel(r, rhs[lv]))
            if pas == 2 and m:
                a_phi, a_z = (ap, ad) if mut == 'ap_ad_swapped' else (ad, ap)
                zn = ph.update(g['z'][k], dz, a_z)[0]
                worst = max(worst, rel(zn, np.array([bm.X[c][0, 0] + ap * dX[c][0, 0] for c in lin], LD)))
                worst = max(worst, rel(ph.update(g['phi'][k], dphi, a_phi)[0], np.array([bm.S[c][0, 0] + ad * dS[c][0, 0] for c in lin], LD)))
    return float(worst)


# (b) compares quantities that went through a dense solve with cond(T) up to ~1e4 for these models; after the refinement step in extended precision the solution
# carries ~cond * 2^-53 * 2^-11: the right-hand sides and directions agree to 1e3 EPS with margin, a mutation changes them by their own size
TOL_NEWTON = 1e3 * EPS


@pytest.mark.parametrize('mdl', MODELS, ids=lambda m: f"seed{m['seed']}-p{m['p']}")
def test_newton_step_of_the_dense_solve(mdl):
    """(b) the Newton step of a dense solve of the brute-force matrix satisfies the linearised equations; the reference's r_loc (pass 1, pass 2 with sig / phi - corrp
    and the arrow terms 2 w (sig S^-1 - corr)[0, i+1], tr(sig S^-1 - corr) - 1), dz, corrp, arrow dS, dX, acor and the update reproduce its cones"""
    g = _model(**mdl)
    assert newton_mismatch(g, Brute(g)) <= TOL_NEWTON


@pytest.mark.parametrize('mut', MUTATIONS)
def test_mutations_of_the_reference_are_caught(mut):
    """(d) every numerical mutation of profiles/phi_kernel_mutations.txt, applied to the reference, breaks (a) or (b) by orders of magnitude on the model with ragged
    rows and two arrow blocks"""
    g = _model(**MODELS[2])
    bm = Brute(g)
    worst = max(schur_mismatch(g, bm, mut), newton_mismatch(g, bm, mut))
    assert worst > 1e-3, (mut, worst)


def test_swapped_gram_indices_are_the_same_number():
    """the issue's mutation 'GSG indices swapped in T_loc,loc' is an EQUIVALENT mutant: X_r and S_r^-1 are symmetric, so GXG_r and GSG_r are, and
    1/2 (GXG[i,j] GSG[j,i] + GXG[j,i] GSG[i,j]) = 1/2 (GXG[i,j] GSG[i,j] + GXG[j,i] GSG[j,i]) up to the rounding of the Gram products -- no test can tell the two apart
    (profiles/phi_kernel_mutations.txt lists it as such; 'gsg_other_cone' is the mutation of that term that changes the value)"""
    g = _model(**MODELS[2])
    s = _stage(g, 0)
    GXG, GSG = s['GXG'], s['GSG']
    swapped = sum((GXG[r] * GSG[r] + GXG[r].T * GSG[r].T) / 2 for r in (0, 1)) + np.diag(np.asarray(g['z'][0], LD) / np.asarray(g['phi'][0], LD))
    assert np.abs(swapped - ph.rows_block(GXG, GSG, g['phi'][0], g['z'][0])[0]).max() <= 64 * 2.0 ** -64 * float(np.abs(swapped).max())


# ---------------------------------------------------------------------------------------------------------------- (c) the cases of the GPU test on the oracle
def _multipliers(r):
    v = [r['Fg'].ravel() * r['s'] * r['alpha']] if 'Fg' in r else []
    v += [f * r['s'] * r['alpha'] for f in r.get('F', []) if f is not None]
    return np.concatenate(v)


@pytest.mark.parametrize('case', pc.ALL_SHAPES, ids=lambda c: 'nb{}-p{}-nx{}-mb{}-ng{}-nc{}'.format(*c[:6]))
def test_cases_are_in_the_main_phase_at_K(case):
    """every member the solver iterates on: indefinite H; the oracle is still in the main phase at every K of the case; no pivot is frozen on the way (shift = 0);
    for K >= 2 the multipliers have left their starting values by more than 1e-2 relative"""
    prob = pc.make_problem(case)
    Ks = pc.case_K(case)
    for b in range(case[0]):
        lo = np.linalg.eigvalsh(co.symmetrize(prob['H'][b])).min()
        if b not in pc.solved_members(case):
            assert lo > 0
            continue
        assert lo < 0
        kw = pc.oracle_rows(case, b, prob)
        args = (prob['A'][b], prob['B'][b], prob['H'][b])
        trace = []
        r = co.sdp_step1(*args, dict(max_iter=max(Ks)), trace=trace, **kw)
        assert len(trace) >= max(Ks) and all(t['phase'] == 0 for t in trace[:max(Ks)]) and r['shift'] == 0.0
        start = _multipliers(co.sdp_step1(*args, dict(max_iter=0), **kw))
        for K in Ks:
            if K >= 2:
                now = _multipliers(co.sdp_step1(*args, dict(max_iter=K - 1), **kw))
                assert np.linalg.norm(now - start) > 1e-2 * np.linalg.norm(now), (K, 'phi still at its starting value')


@pytest.mark.parametrize('case', pc.CENTER_SHAPES, ids=lambda c: 'nb{}-p{}-nx{}-mb{}-ng{}-nc{}'.format(*c[:6]))
def test_centering_cases_reach_the_centering_phase(case):
    """the centering cases end 'optimal' through the centering phase without a frozen pivot, with at least two centering iterations -- the second is where the device
    may take its first chord step (the oracle refactors every iteration; the GPU test's scouting run asserts that a chord step is taken)"""
    prob = pc.make_problem(case)
    b = pc.solved_members(case)[0]
    trace = []
    r = co.sdp_step1(prob['A'][b], prob['B'][b], prob['H'][b], trace=trace, **pc.oracle_rows(case, b, prob))
    assert r['ipm_status'] == 'optimal' and r['shift'] == 0.0
    assert sum(t['phase'] == 1 for t in trace) >= 2
