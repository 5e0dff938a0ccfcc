"""The problems of tests/test_gpu_phi_kernels.py, shared with tests/test_phi_reference_cpu.py (which checks on the CPU oracle that every one of them is in the main
phase at the iteration the GPU test stops at, without a frozen pivot and with multipliers that have left their starting values).  Host only.

A case is (nb, p, nx, mb, ng, nc, ncnt, rho): nb problems of period p with nx states and mb inputs, ng rows of G_k per stage, room for nc rows of C_k, of which
ncnt[k] are present at stage k (None: Step 1 with G alone, convexify_eq_batch; else convexify_step2_batch), and the weight rho of the norm terms (0 with ncnt:
the rows of C_k are cost-free, no arrow blocks)."""
import numpy as np

import convexify_oracle as co

# the smallest shapes at which the multiplier kernels (tunempc_amd/csrc/tmpc_phi.h) take another path
EQ_P2 = (1, 2, 3, 1, 1, 0, None, 0.0)                         # Step 1 with G, no arrows; p = 2: both edges join the same two stages
EQ_P1 = (1, 1, 3, 1, 1, 0, None, 0.0)                         # p = 1: a + b land in the one P block (k_aug_fill), kn = k
FREE_P5 = (1, 5, 4, 2, 2, 2, (2, 0, 1, 2, 1), 0.0)            # rows of C without norm terms; p = 5: both orientations of the coupling slot; d + nz = 14: one tile
NORM_NX5 = (3, 3, 5, 2, 2, 2, (0, 2, 1), 1e-2)                # norm terms: one arrow block (nc = 0) and two (a0 = ng); d + nz = 21: dp = 32; member 1 is positive definite
#                                                               and leaves at the pre-check: the list is compacted to [0, 2], k_phi_steps / k_phi_update cover every problem
NORM_NG0 = (1, 3, 5, 2, 0, 2, (2, 0, 1), 1e-2)                # ng = 0: one arrow block at a0 = 0; a stage without any row
EQ_NX11 = (1, 3, 11, 1, 1, 0, None, 0.0)                      # d = 66, 64 < dp <= 320: the fused order (k_phi_rhs, k_aug_gather before the factorisation)
SMALL_CASES = [EQ_P2, EQ_P1, FREE_P5, NORM_NX5, NORM_NG0, EQ_NX11]
SMALL_K = (1, 2, 5)
# room for more than 32 rows per stage: k_phi_pre<*, BIGR>; the same problem on a 32-row handle must give the same bits
BIGR_CASE = (1, 3, 4, 2, 2, 31, (3, 0, 2), 1e-2)
BIGR_TWIN_NC = 30
LARGE_CASES = [
    (1, 2, 24, 8, 0, 31, (31, 31), 1e-2),                     # the stage of the benchmark, 31 rows under one norm term: arrow block 32 x 32, the full LDS slot
    (1, 2, 30, 4, 1, 0, None, 0.0),                           # n = 34: the <BIGN> forms and kb_phi_dm
    (1, 2, 30, 4, 17, 16, (16, 16), 1e-2),                    # n = 34 with 33 rows present: <BIGN, BIGR>
]
LARGE_K = (3,)
CENTER_SHAPES = [FREE_P5, NORM_NX5]
DEFINITE_MEMBER = {NORM_NX5: 1}

SEEDS = {EQ_P2: 5102, EQ_P1: 5204, FREE_P5: 5300, NORM_NX5: 5400, NORM_NG0: 5500, EQ_NX11: 5600, BIGR_CASE: 5700,
         LARGE_CASES[0]: 5800, LARGE_CASES[1]: 5900, LARGE_CASES[2]: 6000}

# (case, K or 'center' / 'chord', generic stage kernels)
MAIN_CASES = ([(c, k, False) for c in SMALL_CASES for k in SMALL_K] + [(c, k, True) for c in SMALL_CASES for k in SMALL_K]
              + [(BIGR_CASE, k, False) for k in SMALL_K] + [(c, k, False) for c in LARGE_CASES for k in LARGE_K])
CENTER_CASES = [(c, kind, False) for c in CENTER_SHAPES for kind in ('center', 'chord')]
ALL_SHAPES = SMALL_CASES + [BIGR_CASE] + LARGE_CASES


def case_K(case):
    return LARGE_K if case in LARGE_CASES else SMALL_K


def make_problem(case):
    """-> dict(A, B, H [nb, p, ...], J [nb, p, ng + nc, n] (rows of G_k, then of C_k, zero padding), ncnt [nb, p] int32 or None, rho)"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    n = nx + mb
    seed = SEEDS[case]
    members = [co.gen_problem(seed + b, p, nx, mb) for b in range(nb)]
    A = np.stack([m[0] for m in members]); B = np.stack([m[1] for m in members]); H = np.stack([m[2] for m in members])
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


def stage_layout(case, k):
    """rows present at stage k and its arrow blocks [(a0, m)]: one over the rows of G (if any), one over the rows of C present, both only with rho > 0"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    ncs = 0 if ncnt is None else ncnt[k]
    arrows = []
    if ncnt is not None and rho > 0.0:
        if ng:
            arrows.append((0, ng))
        if ncs:
            arrows.append((ng, ncs))
    return ng + ncs, arrows


def oracle_rows(case, b, prob=None):
    """the arguments G=, C=, rho= of convexify_oracle.sdp_step1 for member b"""
    nb, p, nx, mb, ng, nc, ncnt, rho = case
    prob = prob or make_problem(case)
    J = prob['J'][b]
    kw = dict(G=J[:, :ng] if ng else None)
    if ncnt is not None:
        kw['C'] = [J[k, ng:ng + ncnt[k]] if ncnt[k] else None for k in range(p)]
        kw['rho'] = rho
    return kw
