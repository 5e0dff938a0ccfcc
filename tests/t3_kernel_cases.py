"""The problems of tests/test_gpu_t3_kernels.py, shared with tests/test_t3_reference_cpu.py (which checks on the CPU oracle that every one of them is in the main
phase at the iteration the GPU test stops at, without a frozen pivot and with a theta that has left its starting value).  Host only.

A case is (nb, p, nx, mb, ng, nc, ncnt, rho): nb problems of period p with nx states and mb inputs, the Step 3 model (T_k symmetric with every entry > 0,
rho ||T_k||_F in the objective), ng rows of G_k per stage and room for nc rows of C_k of which ncnt[k] are present at stage k (ng = nc = 0:
convexify_step3_batch; else convexify_step3_con_batch, ncnt None: G alone).  n = nx + mb, m = n (n + 1) / 2 entries of T_k, Schur blocks of d + nz + m + 1."""
import numpy as np

import convexify_oracle as co

# the smallest shapes at which the Step 3 kernels (tunempc_amd/csrc/tmpc_t3.h) take another path
P2 = (1, 2, 2, 1, 0, 0, None, 1e-3)                           # n = 3, m = 6, block 10, dp = 16: the small-block factorisation; p = 2: both edges join the same stages
P1 = (1, 1, 3, 1, 0, 0, None, 1e-2)                           # p = 1: a + b land in the one P block, kn = k
P5 = (1, 5, 2, 2, 0, 0, None, 1.0)                            # p = 5: both orientations of the coupling slot; rho = 1: x0 n / wr < 1, so theta starts below 1 (ph < 1)
NB3 = (3, 3, 3, 2, 0, 0, None, 1e-1)                          # member 1 is positive definite and leaves at the pre-check: compacted list, the PH_DONE early returns
M66 = (1, 2, 8, 3, 0, 0, None, 1e-2)                          # n = 11, m = 66 > 64, m + 1 = 67, block 103: second trip of every wave-strided loop; the LDS-DMA factorisation
ROWS_G = (1, 2, 3, 1, 1, 0, None, 1e-2)                       # G only: oT = d + nz > d, k_t3_cross, Q_RPHI2 += after k_phi_pre
ROWS_GC = (1, 3, 3, 2, 1, 2, (2, 0, 1), 1e-2)                 # G + C with norm terms, a stage without any row of C
ROWS_C0 = (1, 3, 3, 2, 0, 2, (2, 0, 1), 1e-2)                 # no rows of G: stage 1 has no row at all while the call has rows (Q_RPHI2 += on what k_phi_pre set for an empty stage)
SMALL_CASES = [P2, P1, P5, NB3, M66, ROWS_G, ROWS_GC, ROWS_C0]
SMALL_K = (1, 2, 5)
N32 = (1, 2, 4, 28, 0, 0, None, 1e-2)                         # n = 32, m = 528: the full 32 x 33 LDS slots of k_t3_schur<false>
N34 = (1, 2, 4, 30, 0, 0, None, 1e-2)                         # n = 34: k_t3_schur<true>, kb_stage_*
LARGE_CASES = [N32, N34]
LARGE_K = (3,)
CENTER_SHAPES = [P5, ROWS_GC]
DEFINITE_MEMBER = {NB3: 1}

SEEDS = {P2: 300, P1: 7205, P5: 7302, NB3: 7400, M66: 7500, ROWS_G: 7603, ROWS_GC: 7700, ROWS_C0: 7700, N32: 7800, N34: 7900}

# (case, K or 'center' / 'chord', generic stage kernels)
MAIN_CASES = ([(c, k, False) for c in SMALL_CASES for k in SMALL_K] + [(c, k, True) for c in SMALL_CASES for k in SMALL_K]
              + [(c, k, False) for c in LARGE_CASES for k in LARGE_K])
CENTER_CASES = [(c, kind, False) for c in CENTER_SHAPES for kind in ('center', 'chord')]
ALL_SHAPES = SMALL_CASES + LARGE_CASES


def case_K(case):
    return LARGE_K if case in LARGE_CASES else SMALL_K


def make_problem(case):
    """-> dict(A, B, H [nb, p, ...], J [nb, p, ng + nc, n] (rows of G_k, then of C_k, zero padding), ncnt [nb, p] int32 or None, rho)"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    n = nx + mb
    seed = SEEDS[case]
    members = [co.gen_problem(seed + b, p, nx, mb) for b in range(nb)]
    A = np.stack([m[0] for m in members]); B = np.stack([m[1] for m in members]); H = np.stack([co.symmetrize(m[2]) for m in members])
    if case in DEFINITE_MEMBER:
        b = DEFINITE_MEMBER[case]
        H[b] = co.symmetrize(members[b][4])
    rng = np.random.default_rng(seed + 77)
    J = np.zeros((nb, p, ng + nc, n))
    J[:, :, :ng] = rng.standard_normal((nb, p, ng, n))
    if ncnt is not None:
        for b in range(nb):
            for k in range(p):
                J[b, k, ng:ng + ncnt[k]] = rng.standard_normal((ncnt[k], n))
    return dict(A=A, B=B, H=H, J=J, ncnt=None if ncnt is None else np.tile(np.asarray(ncnt, np.int32), (nb, 1)), rho=rho)


def solved_members(case):
    return [b for b in range(case[0]) if DEFINITE_MEMBER.get(case) != b]


def oracle_rows(case, b, prob=None):
    """the keyword arguments of convexify_oracle.sdp_step1 for member b of the case (Step 3: force=True)"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    prob = prob or make_problem(case)
    J = prob['J'][b]
    kw = dict(rho=rho, force=True)
    if ng:
        kw['G'] = J[:, :ng]
    if ncnt is not None:
        kw['C'] = [J[k, ng:ng + ncnt[k]] if ncnt[k] else None for k in range(p)]
    return kw


def stage_layout(case, k):
    """rows of [G_k; C_k] present at stage k and the arrow blocks [(a0, m)] of their norm terms (tests/phi_kernel_cases.py: the same multiplier kernels serve Step 3)"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    ncs = 0 if ncnt is None else ncnt[k]
    arrows = []
    if ncnt is not None and rho > 0.0:
        if ng:
            arrows.append((0, ng))
        if ncs:
            arrows.append((ng, ncs))
    return ng + ncs, arrows
