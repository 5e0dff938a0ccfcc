"""The problems of tests/test_gpu_schur_assembly.py, shared with tests/test_schur_reference_cpu.py (which checks on the CPU oracle that every one of them is
still in the main phase at the iteration the GPU test stops at).  Host only."""
import numpy as np

import convexify_oracle as co

# (nb, p, nx, mb): the smallest shapes at which the assembly takes another path, and the iterations K the solve is stopped at
SMALL_CASES = [
    (1, 2, 1, 1),      # d = 1
    (1, 1, 2, 1),      # p = 1: km = k, the coupling block joins a stage to itself
    (1, 2, 3, 1),      # p = 2: both edges join the same two stages
    (3, 3, 5, 2),      # one 16 x 16 tile (small-block factorisation); member 1 is positive definite and leaves at the pre-check: the active list is [0, 2]
    (2, 5, 10, 3),     # d = 55, dp = 64; both storage orientations of the coupling blocks at p = 5
]
SMALL_K = (1, 2, 5)
LARGE_CASES = [
    (1, 3, 24, 8),     # the stage of the benchmark: d = 300, dp = 304, one column pass of k_schur
    (1, 2, 25, 7),     # d = 325, dp = 336 > 320 threads: two column passes
    (1, 2, 31, 1),     # d = dp = 496: no padding rows
    (1, 2, 44, 4),     # n = 48: the generic stage kernels and k_schur with its factor records in global memory (nx > 43)
]
LARGE_K = (3,)
SEEDS = {(1, 2, 1, 1): 4260, (1, 1, 2, 1): 4200, (1, 2, 3, 1): 4070, (3, 3, 5, 2): 4400, (2, 5, 10, 3): 4500,
         (1, 3, 24, 8): 4600, (1, 2, 25, 7): 4700, (1, 2, 31, 1): 4800, (1, 2, 44, 4): 4900}
CASES = [(s, k) for s in SMALL_CASES for k in SMALL_K] + [(s, k) for s in LARGE_CASES for k in LARGE_K]
# (seeds whose H is indefinite for every member the solver iterates on, and which the oracle keeps in the main phase for seven iterations or more:
# tests/test_schur_reference_cpu.py checks both)
DEFINITE_MEMBER = {(3, 3, 5, 2): 1}       # batch member whose H is positive definite (pre-check exit, convexifier.py:82-85)


def make_problem(shape):
    """A, B, H of the batch [nb, p, ...]; members of DEFINITE_MEMBER get the positive definite Hhat of the generator as H"""
    nb, p, nx, mb = shape
    seed = SEEDS[shape]
    members = [co.gen_problem(seed + b, p, nx, mb) for b in range(nb)]
    A = np.stack([m[0] for m in members]); B = np.stack([m[1] for m in members]); H = np.stack([m[2] for m in members])
    if shape in DEFINITE_MEMBER:
        b = DEFINITE_MEMBER[shape]
        H[b] = co.symmetrize(members[b][4])
    return A, B, H


def solved_members(shape):
    return [b for b in range(shape[0]) if DEFINITE_MEMBER.get(shape) != b]
