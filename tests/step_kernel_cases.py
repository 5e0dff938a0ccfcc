"""The cases of tests/test_gpu_step_kernels.py, shared with tests/test_step_reference_cpu.py, and the indices of the workspace scalars both use.  Host only."""
from schur_assembly_cases import LARGE_CASES, LARGE_K, SMALL_CASES, SMALL_K

# per-problem double scalars, per-problem ints and per-stage partial sums: the P_*, I_* and Q_* enums of tunempc_amd/csrc/tmpc_common.h
P_TAU, P_ALPHA, P_S0, P_X0, P_MU, P_MUT, P_SIGMU, P_AP, P_AD = 0, 1, 2, 3, 4, 5, 6, 7, 8
P_PINF, P_DINF, P_STEPN, P_DTAU, P_DALPHA, P_RD0, P_CORR0 = 11, 12, 14, 16, 17, 20, 21
P_BTT, P_BTA, P_BAA, P_SB00, P_SB01, P_SB11, P_SXS, P_RAWSTEP, PS = 23, 24, 25, 26, 27, 28, 31, 40, 48
I_PHASE, I_ITERS, I_NSHIFT, I_CHOLBAD, I_SHIFT0, I_REG, I_CHORD, I_LOWP, IS = 0, 1, 5, 8, 9, 12, 13, 19, 24
Q_TRT2, Q_HBG, Q_DXS, Q_XDS, Q_DXDS, Q_DP2, Q_P2, Q_DH2, Q_M2, NPART = 8, 9, 12, 13, 14, 15, 16, 22, 23, 26
PH_MAIN, PH_CENTER, PH_DONE = 0, 1, 2
TRACE_LEN, TRACE_W = 80, 10
CENTER_DAMP, CHORD_STEP = 0.95, 10.0            # TMPC_CENTER_DAMP; the default of TMPC_TUNE_CHORD_STEP (tmpc_api.hip: h->opt.chord_step)

# main phase: (shape, K, generic stage kernels); the shapes and seeds of tests/schur_assembly_cases.py
MAIN_CASES = ([(s, k, False) for s in SMALL_CASES for k in SMALL_K] + [(s, k, True) for s in SMALL_CASES for k in SMALL_K] + [(s, k, False) for s in LARGE_CASES for k in LARGE_K])
# centering: the iteration is found by a scouting run on the device ('center': the first centering iteration of the first solved member, 'chord': its first chord step)
CENTER_SHAPES = [(3, 3, 5, 2), (2, 5, 10, 3), (1, 3, 24, 8)]
CENTER_CASES = [(s, kind, False) for s in CENTER_SHAPES for kind in ('center', 'chord')]


def eig_thresholds(phase):
    """the thresholds theta of k_eigmin's pre-test in pass 2, longest first (eigmin_body)"""
    if phase == PH_MAIN:
        return [(1.0 / 0.9) * (1.0 + 1e-9)]
    return [CHORD_STEP * (1.0 + 1e-9), (1.0 / CENTER_DAMP) * (1.0 + 1e-9)]
