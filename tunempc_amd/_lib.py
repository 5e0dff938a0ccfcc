"""ctypes binding of the C ABI in include/tunempc_hip.h (libtunempc_hip.so, built in-tree by
`__graft_entry__.build()` / `tunempc_amd/build.py`).  No torch types cross this boundary: plain pointers
and sizes.  The loader fails loudly when the library is missing -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

INFO_STRIDE = 16
FLAG_NO_MFMA = 1
FLAG_PROFILE = 2
FLAG_FAST_EXIT = 4      # stop after the first full centering step (see include/tunempc_hip.h): faster, not reproducible to 1e-8
STATUS_NAMES = {0: 'Optimal', 1: 'Feasible', 2: 'Infeasible'}

# every symbol declared in include/tunempc_hip.h (the drop-in boundary) ...
ARROW_LD = 32       # tunempc_hip.h: TMPC_ARROW_LD
EXPORTS = [
    'tmpc_device_count', 'tmpc_workspace_bytes', 'tmpc_workspace_bytes_eq', 'tmpc_workspace_bytes_con',
    'tmpc_create', 'tmpc_create_eq', 'tmpc_create_con', 'tmpc_destroy', 'tmpc_get_chunk', 'tmpc_set_options', 'tmpc_set_tight', 'tmpc_set_tuning', 'tmpc_create_ex',
    'tmpc_convexify_batch_host', 'tmpc_convexify_batch_device', 'tmpc_convexify_eq_batch_host', 'tmpc_convexify_step2_batch_host',
    'tmpc_convexify_con_batch_device', 'tmpc_workspace_bytes_step3', 'tmpc_create_step3', 'tmpc_convexify_step3_batch_host', 'tmpc_workspace_bytes_step3_con', 'tmpc_create_step3_con', 'tmpc_convexify_step3_con_batch_host', 'tmpc_convexify_step3_batch_device', 'tmpc_convexify_step3_con_batch_device', 'tmpc_supplement_batch_host', 'tmpc_supplement_terms_batch_host',
    'tmpc_tracking_reference_host', 'tmpc_eig_scan_host', 'tmpc_get_profile', 'tmpc_get_trace', 'tmpc_get_dual_host', 'tmpc_get_dual_con_host', 'tmpc_pack_sensitivities_host', 'tmpc_eig_clip_host',
    'tmpc_periodic_lqr_batch_host', 'tmpc_periodic_lqr_batch_device', 'tmpc_periodic_lqr_rows_batch_host', 'tmpc_periodic_lqr_rows_batch_device',
    'tmpc_periodic_lqr_ctg_batch_host', 'tmpc_periodic_lqr_ctg_batch_device', 'tmpc_horizon_lqr_batch_host', 'tmpc_horizon_lqr_batch_device',
    'tmpc_closed_loop_batch_host', 'tmpc_closed_loop_batch_device', 'tmpc_mpc_qp_batch_host', 'tmpc_mpc_qp_batch_device',
    'tmpc_mpc_qp_soft_batch_host', 'tmpc_mpc_qp_soft_batch_device', 'tmpc_mpc_qp_eq_batch_host', 'tmpc_mpc_qp_eq_batch_device',
    'tmpc_mpc_qp_aff_batch_host', 'tmpc_mpc_qp_aff_batch_device', 'tmpc_mpc_qp_quad_batch_host', 'tmpc_mpc_qp_quad_batch_device',
    'tmpc_mpc_qp_warm_batch_host', 'tmpc_mpc_qp_warm_batch_device', 'tmpc_mpc_qp_gain_batch_host', 'tmpc_mpc_qp_gain_batch_device',
    'tmpc_periodic_qp_batch_host', 'tmpc_periodic_qp_batch_device', 'tmpc_periodic_qp_soft_batch_host', 'tmpc_periodic_qp_soft_batch_device',
    'tmpc_last_error', 'tmpc_version',
]
# ... and in include/tunempc_hip_debug.h (unit-test / diagnostic entries)
DEBUG_EXPORTS = [
    'tmpc_debug_gemm_nt', 'tmpc_debug_block_solve', 'tmpc_debug_cr_schedule', 'tmpc_debug_get_multipliers', 'tmpc_debug_get_array',
    'tmpc_debug_min_eig', 'tmpc_debug_min_eig_lane', 'tmpc_debug_factor_bench', 'tmpc_debug_block_factor',
    'tmpc_debug_last_trsm_pairs', 'tmpc_debug_set_stop_iteration', 'tmpc_debug_set_stop_point', 'tmpc_debug_get_iprob',
    'tmpc_debug_soc_step',
]
FLAG_DEBUG_NO_DMA = 32      # tunempc_hip_debug.h: TMPC_DEBUG_FLAG_NO_DMA
# mode bits of tmpc_debug_block_factor (tunempc_hip_debug.h)
FACTOR_PASS1, FACTOR_FUSE_FWD1, FACTOR_LOWP_TRSM, FACTOR_DD = 1, 2, 4, 8


class _FactorIO(C.Structure):
    _fields_ = ([(n, C.POINTER(C.c_double)) for n in ('D', 'Ccpl', 'Dlo', 'Clo', 'rhs')] + [(n, C.POINTER(C.c_int32)) for n in ('list', 'lowp')] +
                [(n, C.POINTER(C.c_double)) for n in ('oD', 'oO', 'oF', 'oDdiag', 'oX')] + [('oO32', C.POINTER(C.c_float))] +
                [(n, C.POINTER(C.c_double)) for n in ('oDl', 'oOl', 'oFl', 'oXl')] + [(n, C.POINTER(C.c_int32)) for n in ('nshift', 'dims', 'orient')])


def library_path():
    """The in-tree build; TMPC_LIB names another build of the same library (A/B measurements of two builds on one box)."""
    return os.environ.get('TMPC_LIB') or os.path.join(_HERE, 'lib', 'libtunempc_hip.so')


def load_library():
    """Load libtunempc_hip.so (never initialises a device by itself)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"tunempc_amd: HIP library not built ({path}); run `python -c 'import __graft_entry__ as g; g.build()'`"
            " -- there is no CPU fallback for the convexify hot path")
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    vp = C.c_void_p
    lib.tmpc_device_count.restype = C.c_int
    lib.tmpc_workspace_bytes.restype = C.c_uint64
    lib.tmpc_workspace_bytes.argtypes = [C.c_int] * 4
    lib.tmpc_workspace_bytes_eq.restype = C.c_uint64
    lib.tmpc_workspace_bytes_eq.argtypes = [C.c_int] * 5
    lib.tmpc_create_eq.restype = C.c_int
    lib.tmpc_create_eq.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_convexify_eq_batch_host.restype = C.c_int
    lib.tmpc_convexify_eq_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.tmpc_workspace_bytes_con.restype = C.c_uint64
    lib.tmpc_workspace_bytes_con.argtypes = [C.c_int] * 6
    lib.tmpc_create_con.restype = C.c_int
    lib.tmpc_create_con.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_convexify_step2_batch_host.restype = C.c_int
    lib.tmpc_convexify_step2_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp, ip, C.c_double, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.tmpc_workspace_bytes_step3.restype = C.c_uint64
    lib.tmpc_workspace_bytes_step3.argtypes = [C.c_int] * 4
    lib.tmpc_create_step3.restype = C.c_int
    lib.tmpc_create_step3.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_workspace_bytes_step3_con.restype = C.c_uint64
    lib.tmpc_workspace_bytes_step3_con.argtypes = [C.c_int] * 6
    lib.tmpc_create_step3_con.restype = C.c_int
    lib.tmpc_create_step3_con.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_convexify_step3_con_batch_host.restype = C.c_int
    lib.tmpc_convexify_step3_con_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp, ip, C.c_double, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.tmpc_convexify_step3_batch_host.restype = C.c_int
    lib.tmpc_convexify_step3_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, C.c_double, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.tmpc_debug_get_multipliers.restype = C.c_int
    lib.tmpc_debug_get_multipliers.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp]
    lib.tmpc_debug_get_array.restype = C.c_int
    lib.tmpc_debug_get_array.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, dp]
    lib.tmpc_debug_set_stop_iteration.restype = C.c_int
    lib.tmpc_debug_set_stop_iteration.argtypes = [vp, C.c_int]
    lib.tmpc_debug_set_stop_point.restype = C.c_int
    lib.tmpc_debug_set_stop_point.argtypes = [vp, C.c_int, C.c_int]
    lib.tmpc_debug_get_iprob.restype = C.c_int
    lib.tmpc_debug_get_iprob.argtypes = [vp, C.c_uint64, C.c_uint64, ip]
    lib.tmpc_convexify_con_batch_device.restype = C.c_int
    lib.tmpc_convexify_con_batch_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_double] + [vp] * 10 + [vp]
    lib.tmpc_convexify_step3_batch_device.restype = C.c_int
    lib.tmpc_convexify_step3_batch_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_double] + [vp] * 10 + [vp]
    lib.tmpc_convexify_step3_con_batch_device.restype = C.c_int
    lib.tmpc_convexify_step3_con_batch_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_double] + [vp] * 11 + [vp]
    lib.tmpc_get_dual_con_host.restype = C.c_int
    lib.tmpc_get_dual_con_host.argtypes = [vp, C.c_int, dp, dp, dp, dp]
    lib.tmpc_create.restype = C.c_int
    lib.tmpc_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_destroy.restype = C.c_int
    lib.tmpc_destroy.argtypes = [vp]
    lib.tmpc_get_chunk.restype = C.c_int
    lib.tmpc_get_chunk.argtypes = [vp]
    lib.tmpc_set_tuning.restype = C.c_int
    lib.tmpc_set_tuning.argtypes = [vp, C.c_int, C.c_double]
    lib.tmpc_create_ex.restype = C.c_int
    lib.tmpc_create_ex.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int] * 8
    lib.tmpc_set_tight.restype = C.c_int
    lib.tmpc_set_tight.argtypes = [vp, C.c_int, C.c_double]
    lib.tmpc_set_options.restype = C.c_int
    lib.tmpc_set_options.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.tmpc_convexify_batch_host.restype = C.c_int
    lib.tmpc_convexify_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.tmpc_convexify_batch_device.restype = C.c_int
    lib.tmpc_convexify_batch_device.argtypes = [vp, C.c_int] + [vp] * 12 + [vp]
    lib.tmpc_supplement_batch_host.restype = C.c_int
    lib.tmpc_supplement_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, dp]
    lib.tmpc_eig_scan_host.restype = C.c_int
    lib.tmpc_eig_scan_host.argtypes = [vp, C.c_int, dp, dp]
    lib.tmpc_eig_clip_host.restype = C.c_int
    lib.tmpc_eig_clip_host.argtypes = [C.c_int, C.c_int, dp, C.c_double, dp, dp, dp, C.POINTER(C.c_int32)]
    lib.tmpc_periodic_lqr_batch_host.restype = C.c_int
    lib.tmpc_periodic_lqr_batch_host.argtypes = [C.c_int] * 4 + [dp] * 4 + [C.c_double, C.c_int] + [dp] * 4
    lib.tmpc_periodic_lqr_batch_device.restype = C.c_int
    lib.tmpc_periodic_lqr_batch_device.argtypes = [C.c_int] * 4 + [vp] * 4 + [C.c_double, C.c_int] + [vp] * 4
    lib.tmpc_periodic_lqr_rows_batch_host.restype = C.c_int
    lib.tmpc_periodic_lqr_rows_batch_host.argtypes = [C.c_int] * 6 + [dp] * 4 + [ip, dp, C.c_double, C.c_int] + [dp] * 5
    lib.tmpc_periodic_lqr_rows_batch_device.restype = C.c_int
    lib.tmpc_periodic_lqr_rows_batch_device.argtypes = [C.c_int] * 6 + [vp] * 6 + [C.c_double, C.c_int] + [vp] * 5
    lib.tmpc_periodic_lqr_ctg_batch_host.restype = C.c_int
    lib.tmpc_periodic_lqr_ctg_batch_host.argtypes = [C.c_int] * 6 + [dp] * 4 + [ip, dp, C.c_double, C.c_double, C.c_int] + [dp] * 4 + [ip, dp]
    lib.tmpc_periodic_lqr_ctg_batch_device.restype = C.c_int
    lib.tmpc_periodic_lqr_ctg_batch_device.argtypes = [C.c_int] * 6 + [vp] * 6 + [C.c_double, C.c_double, C.c_int] + [vp] * 6
    lib.tmpc_horizon_lqr_batch_host.restype = C.c_int
    lib.tmpc_horizon_lqr_batch_host.argtypes = [C.c_int] * 8 + [ip, C.c_int] + [dp] * 4 + [ip, dp, C.c_double] + [dp] * 3 + [ip, dp, ip, dp]
    lib.tmpc_horizon_lqr_batch_device.restype = C.c_int
    lib.tmpc_horizon_lqr_batch_device.argtypes = [C.c_int] * 8 + [ip, C.c_int] + [vp] * 6 + [C.c_double] + [vp] * 7
    lib.tmpc_closed_loop_batch_host.restype = C.c_int
    lib.tmpc_closed_loop_batch_host.argtypes = [C.c_int] * 9 + [dp] * 7 + [ip] + [dp] * 10
    lib.tmpc_closed_loop_batch_device.restype = C.c_int
    lib.tmpc_closed_loop_batch_device.argtypes = [C.c_int] * 9 + [vp] * 18
    lib.tmpc_mpc_qp_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_batch_host.argtypes = [C.c_int] * 9 + [dp] * 6 + [ip, dp, dp, C.c_double, C.c_int] + [dp] * 5 + [ip, ip] + [dp] * 4
    lib.tmpc_mpc_qp_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_batch_device.argtypes = [C.c_int] * 9 + [vp] * 9 + [C.c_double, C.c_int] + [vp] * 11
    lib.tmpc_mpc_qp_soft_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_soft_batch_host.argtypes = lib.tmpc_mpc_qp_batch_host.argtypes + [dp, dp, ip]
    lib.tmpc_mpc_qp_soft_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_soft_batch_device.argtypes = lib.tmpc_mpc_qp_batch_device.argtypes + [vp] * 3
    lib.tmpc_mpc_qp_eq_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_eq_batch_host.argtypes = lib.tmpc_mpc_qp_soft_batch_host.argtypes + [C.c_int, dp, dp, ip, C.c_int, dp, dp, dp, dp]
    lib.tmpc_mpc_qp_eq_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_eq_batch_device.argtypes = lib.tmpc_mpc_qp_soft_batch_device.argtypes + [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.tmpc_mpc_qp_aff_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_aff_batch_host.argtypes = lib.tmpc_mpc_qp_eq_batch_host.argtypes + [dp] * 7
    lib.tmpc_mpc_qp_aff_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_aff_batch_device.argtypes = lib.tmpc_mpc_qp_eq_batch_device.argtypes + [vp] * 7
    lib.tmpc_mpc_qp_quad_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_quad_batch_host.argtypes = lib.tmpc_mpc_qp_aff_batch_host.argtypes + [dp]
    lib.tmpc_mpc_qp_quad_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_quad_batch_device.argtypes = lib.tmpc_mpc_qp_aff_batch_device.argtypes + [vp]
    lib.tmpc_mpc_qp_warm_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_warm_batch_host.argtypes = lib.tmpc_mpc_qp_quad_batch_host.argtypes + [C.c_int, C.c_double] + [dp] * 6 + [ip]
    lib.tmpc_mpc_qp_warm_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_warm_batch_device.argtypes = lib.tmpc_mpc_qp_quad_batch_device.argtypes + [C.c_int, C.c_double] + [vp] * 7
    lib.tmpc_mpc_qp_gain_batch_host.restype = C.c_int
    lib.tmpc_mpc_qp_gain_batch_host.argtypes = [C.c_int] * 11 + [dp] * 5 + [ip] + [dp] * 4 + [ip] + [dp] * 5 + [ip, C.c_double] + [dp] * 3 + [ip, dp, ip, dp, dp, ip, dp, dp]
    lib.tmpc_mpc_qp_gain_batch_device.restype = C.c_int
    lib.tmpc_mpc_qp_gain_batch_device.argtypes = [C.c_int] * 11 + [vp] * 17 + [C.c_double] + [vp] * 11
    lib.tmpc_periodic_qp_batch_host.restype = C.c_int
    lib.tmpc_periodic_qp_batch_host.argtypes = [C.c_int] * 7 + [dp] * 6 + [ip, dp, dp, dp, ip, C.c_double, C.c_int] + [dp] * 7
    lib.tmpc_periodic_qp_batch_device.restype = C.c_int
    lib.tmpc_periodic_qp_batch_device.argtypes = [C.c_int] * 7 + [vp] * 11 + [C.c_double, C.c_int] + [vp] * 7
    lib.tmpc_periodic_qp_soft_batch_host.restype = C.c_int
    lib.tmpc_periodic_qp_soft_batch_host.argtypes = [C.c_int] * 7 + [dp] * 6 + [ip, dp, dp, dp, dp, dp, ip, C.c_double, C.c_int] + [dp] * 6 + [ip, dp, dp]
    lib.tmpc_periodic_qp_soft_batch_device.restype = C.c_int
    lib.tmpc_periodic_qp_soft_batch_device.argtypes = [C.c_int] * 7 + [vp] * 13 + [C.c_double, C.c_int] + [vp] * 9
    lib.tmpc_get_profile.restype = C.c_int
    lib.tmpc_get_profile.argtypes = [vp, dp]
    lib.tmpc_get_trace.restype = C.c_int
    lib.tmpc_get_trace.argtypes = [vp, C.c_int, dp]
    lib.tmpc_pack_sensitivities_host.restype = C.c_int
    lib.tmpc_pack_sensitivities_host.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.c_double, C.c_int, dp, ip, ip, dp, dp]
    lib.tmpc_get_dual_host.restype = C.c_int
    lib.tmpc_get_dual_host.argtypes = [vp, C.c_int, dp, dp, dp]
    lib.tmpc_debug_gemm_nt.restype = C.c_int
    lib.tmpc_debug_gemm_nt.argtypes = [vp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.tmpc_debug_block_solve.restype = C.c_int
    lib.tmpc_debug_block_solve.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, ip]
    lib.tmpc_supplement_terms_batch_host.restype = C.c_int
    lib.tmpc_supplement_terms_batch_host.argtypes = [vp, C.c_int, dp, dp, dp, C.c_int, dp, dp, dp, dp]
    lib.tmpc_tracking_reference_host.restype = C.c_int
    lib.tmpc_tracking_reference_host.argtypes = [vp, C.c_int, dp, dp, dp, C.c_double, dp, dp, ip]
    lib.tmpc_debug_cr_schedule.restype = C.c_int
    lib.tmpc_debug_cr_schedule.argtypes = [C.c_int, ip, C.c_int]
    lib.tmpc_debug_block_factor.restype = C.c_int
    lib.tmpc_debug_block_factor.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_FactorIO)]
    lib.tmpc_debug_factor_bench.restype = C.c_int
    lib.tmpc_debug_factor_bench.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    lib.tmpc_debug_last_trsm_pairs.restype = C.c_longlong
    lib.tmpc_debug_last_trsm_pairs.argtypes = []
    lib.tmpc_debug_min_eig.restype = C.c_int
    lib.tmpc_debug_min_eig.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    lib.tmpc_debug_soc_step.restype = C.c_int
    lib.tmpc_debug_soc_step.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
    lib.tmpc_debug_min_eig_lane.restype = C.c_int
    lib.tmpc_debug_min_eig_lane.argtypes = [vp, C.c_int, C.c_int, dp, dp]
    lib.tmpc_last_error.restype = C.c_char_p
    lib.tmpc_version.restype = C.c_char_p
    _LIB = lib
    return lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


class EigNotConverged(RuntimeError):
    """tmpc_eig_clip_host returned TMPC_E_NOCONV: the Jacobi sweeps were exhausted; `.partial` holds the last iterate."""


E_NOCONV = -6
E_UNSUPPORTED = -2
LQR_INFO_STRIDE = 8
LQR_CTG_INFO_STRIDE = 12
CLOSED_LOOP_INFO_STRIDE = 4
MPC_QP_INFO_STRIDE = 8
PERIODIC_QP_INFO_STRIDE = 8
PERIODIC_QP_RES_STRIDE = 4
PERIODIC_QP_SOFT_RES_STRIDE = 6


def _check(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"tunempc_amd: {what} failed with code {rc}: {lib.tmpc_last_error().decode()}")


# which-codes of tmpc_debug_get_array for the row state of the multiplier kernels (csrc/tmpc_phi.h); the arrow arrays are [B,p,2,ARROW_LD,ARROW_LD]
DEBUG_ARRAY_CODES = dict(psm=0, pvec=1, G=42, corrp=43, at=44, adt=45, aX=46, adX=47, acor=48, aSi=49, aLi=50, aLXi=51, asum=52, prs=53)
ARROW_LD = 32


class HipConvexifier:
    """Handle for batched convexification of problems of one shape (p, nx, mb) on the current HIP device."""

    def __init__(self, p, nx, mb, chunk=0, tol=None, center_tol=None, max_iter=None, center_iter=None, flags=0, ng=0, nc=0, step3=False, lanes=0):
        self.lib = load_library()
        if self.lib.tmpc_device_count() < 1:
            raise RuntimeError("tunempc_amd: no HIP device visible; the convexify hot path has no CPU fallback")
        self.p, self.nx, self.mb, self.n = int(p), int(nx), int(mb), int(nx) + int(mb)
        self._h = C.c_void_p()
        self.ng = int(ng)     # rows of the equality-constraint Jacobian per stage (convexifier.py:249-255), 0: none
        self.nc = int(nc)     # room for active-constraint rows per stage (Step 2, convexifier.py:258-266), 0: none
        self.step3 = bool(step3)      # room for the regularisation T_k of Step 3 (convexifier.py:137-147); such a handle also serves the plain model
        if lanes:
            _check(self.lib, self.lib.tmpc_create_ex(C.byref(self._h), int(chunk), self.p, self.nx, self.mb, self.ng, self.nc, int(self.step3), int(lanes)), 'tmpc_create_ex')
        elif self.step3 and (self.ng or self.nc):
            _check(self.lib, self.lib.tmpc_create_step3_con(C.byref(self._h), int(chunk), self.p, self.nx, self.mb, self.ng, self.nc), 'tmpc_create_step3_con')
        elif self.step3:
            _check(self.lib, self.lib.tmpc_create_step3(C.byref(self._h), int(chunk), self.p, self.nx, self.mb), 'tmpc_create_step3')
        else:
            _check(self.lib, self.lib.tmpc_create_con(C.byref(self._h), int(chunk), self.p, self.nx, self.mb, self.ng, self.nc), 'tmpc_create_con')
        self.chunk = int(self.lib.tmpc_get_chunk(self._h))
        self.flags = int(flags)
        self.set_options(tol, center_tol, max_iter, center_iter, flags)

    def set_options(self, tol=None, center_tol=None, max_iter=None, center_iter=None, flags=None):
        if flags is not None:
            self.flags = int(flags)
        _check(self.lib, self.lib.tmpc_set_options(self._h, float(tol or 0.0), float(center_tol or 0.0),
                                                   int(max_iter or 0), int(center_iter or 0), self.flags), 'tmpc_set_options')

    def set_tuning(self, chord_step=None, small_blocks=None, eig_pretest=None, fuse_fwd=None, graph=None, persistent=None, lowp_switch=None, lowp_trsm=None, trsm_pair=None):
        """Performance knobs of the handle (include/tunempc_hip.h: tmpc_set_tuning); None keeps the current value."""
        for key, v in ((1, chord_step), (2, small_blocks), (3, eig_pretest), (4, fuse_fwd), (5, graph), (7, persistent), (8, lowp_switch), (9, lowp_trsm), (10, trsm_pair)):
            if v is not None:
                _check(self.lib, self.lib.tmpc_set_tuning(self._h, key, float(v)), 'tmpc_set_tuning')

    def set_tight(self, enable=True, tight_tol=None):
        """Tight-accuracy mode (include/tunempc_hip.h: tmpc_set_tight): continue every Optimal problem towards tight_tol * kappa (default 2^-37)
        with double-double block linear algebra and a dd dual-Newton polish.  Step 1 and Step 2 handles (nx <= 51; with rows of G / C while
        rows * (2 n + 2 nx) <= 4040); Step 3 handles are refused (RuntimeError from TMPC_E_UNSUPPORTED)."""
        _check(self.lib, self.lib.tmpc_set_tight(self._h, 1 if enable else 0, float(tight_tol or 0.0)), 'tmpc_set_tight')

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.tmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ host-buffer entry
    def convexify_batch(self, A, B, H):
        """A [nb,p,nx,nx], B [nb,p,nx,mb], H [nb,p,n,n] (numpy, fp64) -> dict of numpy outputs."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64)
        nb = A.shape[0]
        assert A.shape == (nb, self.p, self.nx, self.nx), A.shape
        assert B.shape == (nb, self.p, self.nx, self.mb), B.shape
        assert H.shape == (nb, self.p, self.n, self.n), H.shape
        out = dict(Hc=np.empty_like(H), dHc=np.empty_like(H), P=np.empty_like(A), alpha=np.empty(nb), beta=np.empty(nb),
                   kappa=np.empty(nb), status=np.empty(nb, np.int32), iters=np.empty(nb, np.int32),
                   info=np.empty((nb, INFO_STRIDE)))
        if nb == 0:
            return out          # empty batch: empty outputs, no device call (the C ABI rejects nb < 1)
        rc = self.lib.tmpc_convexify_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(H), _dptr(out['Hc']), _dptr(out['dHc']),
                                                _dptr(out['P']), _dptr(out['alpha']), _dptr(out['beta']), _dptr(out['kappa']),
                                                _iptr(out['status']), _iptr(out['iters']), _dptr(out['info']))
        _check(self.lib, rc, 'tmpc_convexify_batch_host')
        return out

    def convexify_eq_batch(self, A, B, H, G):
        """Step 1 with the equality-constraint term: G [nb,p,ng,n] (ng of the constructor) -> outputs of convexify_batch + Fg [nb,p,ng]."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64); G = np.ascontiguousarray(G, dtype=np.float64)
        nb = A.shape[0]
        assert A.shape == (nb, self.p, self.nx, self.nx), A.shape
        assert B.shape == (nb, self.p, self.nx, self.mb), B.shape
        assert H.shape == (nb, self.p, self.n, self.n), H.shape
        assert self.ng > 0 and G.shape == (nb, self.p, self.ng, self.n), (G.shape, self.ng)
        out = dict(Hc=np.empty_like(H), dHc=np.empty_like(H), P=np.empty_like(A), Fg=np.empty((nb, self.p, self.ng)),
                   alpha=np.empty(nb), beta=np.empty(nb), kappa=np.empty(nb), status=np.empty(nb, np.int32),
                   iters=np.empty(nb, np.int32), info=np.empty((nb, INFO_STRIDE)))
        if nb == 0:
            return out          # empty batch: empty outputs, no device call (the C ABI rejects nb < 1)
        rc = self.lib.tmpc_convexify_eq_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(H), _dptr(G), _dptr(out['Hc']),
                                                   _dptr(out['dHc']), _dptr(out['P']), _dptr(out['Fg']), _dptr(out['alpha']),
                                                   _dptr(out['beta']), _dptr(out['kappa']), _iptr(out['status']),
                                                   _iptr(out['iters']), _dptr(out['info']))
        _check(self.lib, rc, 'tmpc_convexify_eq_batch_host')
        return out

    def debug_array(self, which, offset, count):
        """`count` doubles from `offset` of workspace array `which` of lane 0 (tunempc_hip_debug.h: tmpc_debug_get_array; DEBUG_ARRAY_CODES names the codes of
        the stage-local multipliers).  A code whose array the handle does not have raises RuntimeError (TMPC_E_ARG)."""
        out = np.empty(int(count))
        _check(self.lib, self.lib.tmpc_debug_get_array(self._h, int(which), int(offset), int(count), _dptr(out)), 'tmpc_debug_get_array')
        return out

    def debug_set_stop_iteration(self, k):
        """With flags=8 (TMPC_DEBUG_FLAG_STOP_ASSEMBLED): stop at the assembled system of iteration k (default 1); tunempc_hip_debug.h."""
        _check(self.lib, self.lib.tmpc_debug_set_stop_iteration(self._h, int(k)), 'tmpc_debug_set_stop_iteration')

    def debug_set_stop_point(self, k, point):
        """With flags=8: stop inside iteration k at point 0 (assembled system), 1 (after pass 1 and k_ctrl_b), 2 (pass 2 complete, before k_ctrl_c) or
        3 (iteration complete); tunempc_hip_debug.h: TMPC_DEBUG_STOP_*."""
        _check(self.lib, self.lib.tmpc_debug_set_stop_point(self._h, int(k), int(point)), 'tmpc_debug_set_stop_point')

    def debug_iprob(self, offset, count):
        """`count` int32 from `offset` of the per-problem integer state of lane 0 (iprob [B,24]: the I_* enum of csrc/tmpc_common.h)."""
        out = np.empty(int(count), np.int32)
        _check(self.lib, self.lib.tmpc_debug_get_iprob(self._h, int(offset), int(count), _iptr(out)), 'tmpc_debug_get_iprob')
        return out

    def debug_multipliers(self, nb, nr):
        out = [np.empty((nb, self.p, nr)) for _ in range(4)]
        _check(self.lib, self.lib.tmpc_debug_get_multipliers(self._h, nb, nr, *[_dptr(o) for o in out]), 'tmpc_debug_get_multipliers')
        return dict(phi=out[0], z=out[1], dphi=out[2], dz=out[3])

    def convexify_step2_batch(self, A, B, H, J, ncnt, rho):
        """The Step 2 model (convexifier.py:116-131).  J [nb,p,ng+nc,n]: rows of G_k, then rows of C_k, zero padding;
        ncnt [nb,p] int32: rows of C_k present -> outputs of convexify_batch + FgF [nb,p,ng+nc] (Fg_k, then F_k)."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64); J = np.ascontiguousarray(J, dtype=np.float64)
        ncnt = np.ascontiguousarray(ncnt, dtype=np.int32)
        nb = A.shape[0]
        nr = self.ng + self.nc
        assert A.shape == (nb, self.p, self.nx, self.nx), A.shape
        assert B.shape == (nb, self.p, self.nx, self.mb), B.shape
        assert H.shape == (nb, self.p, self.n, self.n), H.shape
        assert self.nc > 0 and J.shape == (nb, self.p, nr, self.n) and ncnt.shape == (nb, self.p), (J.shape, ncnt.shape, nr)
        out = dict(Hc=np.empty_like(H), dHc=np.empty_like(H), P=np.empty_like(A), FgF=np.empty((nb, self.p, nr)),
                   alpha=np.empty(nb), beta=np.empty(nb), kappa=np.empty(nb), status=np.empty(nb, np.int32),
                   iters=np.empty(nb, np.int32), info=np.empty((nb, INFO_STRIDE)))
        if nb == 0:
            return out          # empty batch: empty outputs, no device call (the C ABI rejects nb < 1)
        rc = self.lib.tmpc_convexify_step2_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(H), _dptr(J), _iptr(ncnt), float(rho),
                                                      _dptr(out['Hc']), _dptr(out['dHc']), _dptr(out['P']), _dptr(out['FgF']),
                                                      _dptr(out['alpha']), _dptr(out['beta']), _dptr(out['kappa']),
                                                      _iptr(out['status']), _iptr(out['iters']), _dptr(out['info']))
        _check(self.lib, rc, 'tmpc_convexify_step2_batch_host')
        return out

    def convexify_step3_batch(self, A, B, H, rho):
        """The Step 3 model (convexifier.py:137-147), plain model + T: outputs of convexify_batch + T [nb,p,n,n] (every entry > 0)."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64)
        nb = A.shape[0]
        assert self.step3, 'handle created without step3=True'
        assert A.shape == (nb, self.p, self.nx, self.nx) and B.shape == (nb, self.p, self.nx, self.mb) and H.shape == (nb, self.p, self.n, self.n)
        out = dict(Hc=np.empty_like(H), dHc=np.empty_like(H), P=np.empty_like(A), T=np.empty_like(H), alpha=np.empty(nb), beta=np.empty(nb),
                   kappa=np.empty(nb), status=np.empty(nb, np.int32), iters=np.empty(nb, np.int32), info=np.empty((nb, INFO_STRIDE)))
        if nb == 0:
            return out
        rc = self.lib.tmpc_convexify_step3_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(H), float(rho), _dptr(out['Hc']), _dptr(out['dHc']),
                                                      _dptr(out['P']), _dptr(out['T']), _dptr(out['alpha']), _dptr(out['beta']), _dptr(out['kappa']),
                                                      _iptr(out['status']), _iptr(out['iters']), _dptr(out['info']))
        _check(self.lib, rc, 'tmpc_convexify_step3_batch_host')
        return out

    def convexify_step3_con_batch(self, A, B, H, J, ncnt, rho):
        """Step 3 with the multipliers of G / C in the same solve (convexifier.py:144): J [nb,p,ng+nc,n] and ncnt [nb,p] as in
        convexify_step2_batch, or J [nb,p,ng,n] with ncnt=None (G only, cost-free multipliers).  Outputs of convexify_batch + FgF + T."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        H = np.ascontiguousarray(H, dtype=np.float64); J = np.ascontiguousarray(J, dtype=np.float64)
        nb = A.shape[0]
        assert self.step3 and self.ng + self.nc > 0, 'handle created without step3=True and constraint rows'
        nr = self.ng + (self.nc if ncnt is not None else 0)
        assert J.shape == (nb, self.p, nr, self.n), (J.shape, (nb, self.p, nr, self.n))
        if ncnt is not None:
            ncnt = np.ascontiguousarray(ncnt, dtype=np.int32)
            assert ncnt.shape == (nb, self.p)
        out = dict(Hc=np.empty_like(H), dHc=np.empty_like(H), P=np.empty_like(A), T=np.empty_like(H), FgF=np.zeros((nb, self.p, nr)), alpha=np.empty(nb),
                   beta=np.empty(nb), kappa=np.empty(nb), status=np.empty(nb, np.int32), iters=np.empty(nb, np.int32), info=np.empty((nb, INFO_STRIDE)))
        if nb == 0:
            return out
        rc = self.lib.tmpc_convexify_step3_con_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(H), _dptr(J), _iptr(ncnt), float(rho), _dptr(out['Hc']),
                                                          _dptr(out['dHc']), _dptr(out['P']), _dptr(out['FgF']), _dptr(out['T']), _dptr(out['alpha']),
                                                          _dptr(out['beta']), _dptr(out['kappa']), _iptr(out['status']), _iptr(out['iters']), _dptr(out['info']))
        _check(self.lib, rc, 'tmpc_convexify_step3_con_batch_host')
        return out

    # ------------------------------------------------------------------ device-resident entry (torch tensors)
    def convexify_batch_device(self, A, B, H, out=None, stream=None):
        """torch CUDA tensors (fp64, contiguous) in, torch tensors out; data stays in HBM."""
        import torch
        nb = A.shape[0]
        for t in (A, B, H):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        dev = A.device
        if out is None:
            out = dict(Hc=torch.empty_like(H), dHc=torch.empty_like(H), P=torch.empty_like(A),
                       alpha=torch.empty(nb, dtype=torch.float64, device=dev), beta=torch.empty(nb, dtype=torch.float64, device=dev),
                       kappa=torch.empty(nb, dtype=torch.float64, device=dev), status=torch.empty(nb, dtype=torch.int32, device=dev),
                       iters=torch.empty(nb, dtype=torch.int32, device=dev),
                       info=torch.empty((nb, INFO_STRIDE), dtype=torch.float64, device=dev))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.tmpc_convexify_batch_device(self._h, nb, ptr(A), ptr(B), ptr(H), ptr(out['Hc']), ptr(out['dHc']), ptr(out['P']),
                                                  ptr(out['alpha']), ptr(out['beta']), ptr(out['kappa']), ptr(out['status']),
                                                  ptr(out['iters']), ptr(out['info']), C.c_void_p(st))
        _check(self.lib, rc, 'tmpc_convexify_batch_device')
        return out

    def convexify_con_batch_device(self, A, B, H, J, ncnt=None, rho=0.0, stream=None):
        """Device-resident Step 1 with G (ncnt None, J = G [nb,p,ng,n]) or Step 2 model (J [nb,p,ng+nc,n], ncnt [nb,p] int32):
        torch CUDA tensors in, torch tensors out (the dict of convexify_batch_device plus 'FgF')."""
        import torch
        nb = A.shape[0]
        for t in (A, B, H, J):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        assert ncnt is None or (ncnt.is_cuda and ncnt.dtype == torch.int32 and ncnt.is_contiguous())
        nr = self.ng if ncnt is None else self.ng + self.nc
        assert tuple(J.shape) == (nb, self.p, nr, self.n), (tuple(J.shape), nr)
        dev = A.device
        f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
        out = dict(Hc=torch.empty_like(H), dHc=torch.empty_like(H), P=torch.empty_like(A), FgF=f64(nb, self.p, nr), alpha=f64(nb), beta=f64(nb),
                   kappa=f64(nb), status=torch.empty(nb, dtype=torch.int32, device=dev), iters=torch.empty(nb, dtype=torch.int32, device=dev),
                   info=f64(nb, INFO_STRIDE))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = self.lib.tmpc_convexify_con_batch_device(self._h, nb, ptr(A), ptr(B), ptr(H), ptr(J), ptr(ncnt) if ncnt is not None else None,
                                                      float(rho), ptr(out['Hc']), ptr(out['dHc']), ptr(out['P']), ptr(out['FgF']),
                                                      ptr(out['alpha']), ptr(out['beta']), ptr(out['kappa']), ptr(out['status']),
                                                      ptr(out['iters']), ptr(out['info']), C.c_void_p(st))
        _check(self.lib, rc, 'tmpc_convexify_con_batch_device')
        return out

    def convexify_step3_batch_device(self, A, B, H, rho, J=None, ncnt=None, stream=None):
        """Device-resident Step 3 (convexifier.py:137-147): torch CUDA tensors in, torch tensors out (the dict of convexify_batch_device plus 'T'); with J
        (and ncnt) the multipliers of G / C ride in the same solve (convexifier.py:144), output 'FgF' as well."""
        import torch
        nb = A.shape[0]
        for t in (A, B, H) + ((J,) if J is not None else ()):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        assert self.step3 and (J is None or self.ng + self.nc > 0)
        assert ncnt is None or (ncnt.is_cuda and ncnt.dtype == torch.int32 and ncnt.is_contiguous())
        dev = A.device
        f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
        out = dict(Hc=torch.empty_like(H), dHc=torch.empty_like(H), P=torch.empty_like(A), T=torch.empty_like(H), alpha=f64(nb), beta=f64(nb), kappa=f64(nb),
                   status=torch.empty(nb, dtype=torch.int32, device=dev), iters=torch.empty(nb, dtype=torch.int32, device=dev), info=f64(nb, INFO_STRIDE))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: C.c_void_p(t.data_ptr())
        if J is None:
            rc = self.lib.tmpc_convexify_step3_batch_device(self._h, nb, ptr(A), ptr(B), ptr(H), float(rho), ptr(out['Hc']), ptr(out['dHc']), ptr(out['P']),
                                                            ptr(out['T']), ptr(out['alpha']), ptr(out['beta']), ptr(out['kappa']), ptr(out['status']),
                                                            ptr(out['iters']), ptr(out['info']), C.c_void_p(st))
            _check(self.lib, rc, 'tmpc_convexify_step3_batch_device')
            return out
        nr = self.ng if ncnt is None else self.ng + self.nc
        assert tuple(J.shape) == (nb, self.p, nr, self.n), (tuple(J.shape), nr)
        out['FgF'] = f64(nb, self.p, nr)
        rc = self.lib.tmpc_convexify_step3_con_batch_device(self._h, nb, ptr(A), ptr(B), ptr(H), ptr(J), ptr(ncnt) if ncnt is not None else None,
                                                            float(rho), ptr(out['Hc']), ptr(out['dHc']), ptr(out['P']), ptr(out['FgF']), ptr(out['T']),
                                                            ptr(out['alpha']), ptr(out['beta']), ptr(out['kappa']), ptr(out['status']), ptr(out['iters']),
                                                            ptr(out['info']), C.c_void_p(st))
        _check(self.lib, rc, 'tmpc_convexify_step3_con_batch_device')
        return out

    def supplement_batch(self, A, B, P):
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        nb = A.shape[0]
        dH = np.empty((nb, self.p, self.n, self.n))
        _check(self.lib, self.lib.tmpc_supplement_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(P), _dptr(dH)), 'tmpc_supplement_batch_host')
        return dH

    def supplement_terms_batch(self, A, B, P, J=None, wts=None, T=None):
        """dHc = sym(calH(P) + J' diag(w) J + T) per stage (convexifier.py:165-211); J [nb,p,nr,n], wts [nb,p,nr], T [nb,p,n,n]."""
        A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        nb, nr = A.shape[0], 0
        if J is not None:
            J = np.ascontiguousarray(J, dtype=np.float64); wts = np.ascontiguousarray(wts, dtype=np.float64)
            nr = J.shape[2]
            assert J.shape == (nb, self.p, nr, self.n) and wts.shape == (nb, self.p, nr), (J.shape, wts.shape)
        if T is not None:
            T = np.ascontiguousarray(T, dtype=np.float64)
            assert T.shape == (nb, self.p, self.n, self.n), T.shape
        dH = np.empty((nb, self.p, self.n, self.n))
        _check(self.lib, self.lib.tmpc_supplement_terms_batch_host(self._h, nb, _dptr(A), _dptr(B), _dptr(P), nr, _dptr(J), _dptr(wts), _dptr(T), _dptr(dH)),
               'tmpc_supplement_terms_batch_host')
        return dH

    def eig_scan(self, H):
        H = np.ascontiguousarray(H, dtype=np.float64)
        nb = H.shape[0]
        out = np.empty((nb, self.p, 4))
        _check(self.lib, self.lib.tmpc_eig_scan_host(self._h, nb, _dptr(H), _dptr(out)), 'tmpc_eig_scan_host')
        return out

    def profile(self):
        out = np.zeros(16)
        _check(self.lib, self.lib.tmpc_get_profile(self._h, _dptr(out)), 'tmpc_get_profile')
        keys = ['pre_ms', 'schur_ms', 'factor_ms', 'pass1_ms', 'pass2_ms', 'factor_launches', 'total_ms', 'ipm_iters',
                'problem_factorisations', 'potrf_ms', 'trsm_ms', 'update_ms', 'lanes', 'lowp_factorisations', 'update_f32_ms', 'persistent_problems']
        return dict(zip(keys, out.tolist()))

    def pack_sensitivities(self, C=None, mu=None, Hbig=None, thr=1e-15, ncmax=None, nb=None):
        """GPU form of the array post-processing of Pocp.get_sensitivities (pocp.py:322-361): C [nb,p,nh,n], mu [nb,p,nh] -> C_As
        [nb,p,ncmax,n] (active rows in order, zero-padded), nc [nb,p], idx [nb,p,nh] (-1 padded), q [nb,p,n]; Hbig [nb,p*n,p*n] ->
        H [nb,p,n,n].  Without C: q = zeros (pass nb)."""
        out = {}
        p, n = self.p, self.n
        if C is not None:
            C = np.ascontiguousarray(C, dtype=np.float64); mu = np.ascontiguousarray(mu, dtype=np.float64)
            nb, nh = C.shape[0], C.shape[2]
            assert C.shape == (nb, p, nh, n) and mu.shape == (nb, p, nh), (C.shape, mu.shape)
            ncmax = int(ncmax or nh)
            out.update(C_As=np.empty((nb, p, ncmax, n)), nc=np.empty((nb, p), np.int32), idx=np.empty((nb, p, nh), np.int32))
        else:
            nh, ncmax = 0, 0
            nb = int(nb if nb is not None else Hbig.shape[0])
        out['q'] = np.empty((nb, p, n))
        if Hbig is not None:
            Hbig = np.ascontiguousarray(Hbig, dtype=np.float64)
            assert Hbig.shape == (nb, p * n, p * n), Hbig.shape
            out['H'] = np.empty((nb, p, n, n))
        _check(self.lib, self.lib.tmpc_pack_sensitivities_host(self._h, nb, nh, _dptr(C), _dptr(mu), _dptr(Hbig), float(thr), ncmax,
                                                               _dptr(out.get('C_As')), _iptr(out.get('nc')), _iptr(out.get('idx')),
                                                               _dptr(out['q']), _dptr(out.get('H'))), 'tmpc_pack_sensitivities_host')
        if 'nc' in out and (out['nc'] > ncmax).any():
            raise ValueError('pack_sensitivities: a stage has %d active rows, more than ncmax = %d' % (int(out['nc'].max()), ncmax))
        return out

    def dual(self, nb):
        """Dual iterate of the last wave solved (plain Step 1 model, scaled problem): dict(X1, X2 [nb,p,n,n], x0, tau, alpha, mu_target [nb]);
        see tmpc_get_dual_host -- the data for a solver-independent bound on the optimality gap of kappa."""
        X1 = np.empty((nb, self.p, self.n, self.n)); X2 = np.empty_like(X1); sc = np.empty((nb, 4))
        _check(self.lib, self.lib.tmpc_get_dual_host(self._h, int(nb), _dptr(X1), _dptr(X2), _dptr(sc)), 'tmpc_get_dual_host')
        return dict(X1=X1, X2=X2, x0=sc[:, 0].copy(), tau=sc[:, 1].copy(), alpha=sc[:, 2].copy(), mu_target=sc[:, 3].copy())

    def dual_con(self, nb, arrows=False):
        """Dual side of the stage-local multipliers of the last wave (tmpc_get_dual_con_host): dict(phi, z [nb,p,ng+nc][, aX [nb,p,2,32,32], at [nb,p,2]])."""
        nr = self.ng + self.nc
        phi = np.zeros((nb, self.p, nr)); z = np.zeros_like(phi)
        aX = np.zeros((nb, self.p, 2, ARROW_LD, ARROW_LD)) if arrows else None; at = np.zeros((nb, self.p, 2)) if arrows else None
        _check(self.lib, self.lib.tmpc_get_dual_con_host(self._h, int(nb), _dptr(phi), _dptr(z), _dptr(aX) if arrows else None, _dptr(at) if arrows else None), 'tmpc_get_dual_con_host')
        out = dict(phi=phi, z=z)
        if arrows:
            out.update(aX=aX, at=at)
        return out

    def trace(self, nb):
        """[nb, 80, 10] per-iteration diagnostics of the last chunk (it, phase, mu, tau, pinf, dinf, ap, ad, step, shifts)."""
        out = np.zeros((nb, 80, 10))
        _check(self.lib, self.lib.tmpc_get_trace(self._h, nb, _dptr(out)), 'tmpc_get_trace')
        return out

    # ------------------------------------------------------------------ unit-test hooks
    def debug_gemm_nt(self, Cm, A, B, mode=0, lower=False):
        Cm = np.ascontiguousarray(Cm, dtype=np.float64).copy(); A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        M, N = Cm.shape; K = A.shape[1]
        _check(self.lib, self.lib.tmpc_debug_gemm_nt(self._h, _dptr(Cm), _dptr(A), _dptr(B), M, N, K, int(mode), int(lower)), 'tmpc_debug_gemm_nt')
        return Cm

    def debug_min_eig(self, W, lane=False):
        """smallest eigenvalues of symmetric matrices [nmat, n, n]; lane=True: the one-thread-per-matrix routine of the small shapes (n <= 8)"""
        W = np.ascontiguousarray(W, dtype=np.float64)
        nmat, n, _ = W.shape
        out = np.empty(nmat)
        fn = self.lib.tmpc_debug_min_eig_lane if lane else self.lib.tmpc_debug_min_eig
        _check(self.lib, fn(self._h, nmat, n, _dptr(W), _dptr(out)), 'tmpc_debug_min_eig')
        return out

    def debug_soc_step(self, u, du):
        """the step length into the second-order cone for pairs (u, du) [nvec, m1] as the "eigenvalue" -1/theta, 0 if unbounded (soc_step_eig of csrc/tmpc_t3.h)"""
        u = np.ascontiguousarray(u, dtype=np.float64); du = np.ascontiguousarray(du, dtype=np.float64)
        nvec, m1 = u.shape
        assert du.shape == u.shape
        out = np.empty(nvec)
        _check(self.lib, self.lib.tmpc_debug_soc_step(self._h, nvec, m1, _dptr(u), _dptr(du), _dptr(out)), 'tmpc_debug_soc_step')
        return out

    def tracking_reference(self, Hc, q, wref, ts):
        """W_k = sym(Hc_k)/ts, yref_k = wref_k - Hc_k^-1 q_k for a stack of stages (pmpc.py:961-974).
        Hc [..., n, n], q/wref [..., n] -> (W [..., n, n], yref [..., n], info [...])."""
        Hc = np.ascontiguousarray(Hc, dtype=np.float64); q = np.ascontiguousarray(q, dtype=np.float64)
        wref = np.ascontiguousarray(wref, dtype=np.float64)
        n = self.nx + self.mb
        if Hc.shape[-2:] != (n, n) or q.shape != Hc.shape[:-1] or wref.shape != q.shape:
            raise ValueError('tracking_reference: expected Hc [..., %d, %d] and q, wref [..., %d]' % (n, n, n))
        ns = int(np.prod(Hc.shape[:-2], dtype=np.int64))
        W = np.empty_like(Hc); yref = np.empty_like(q); info = np.zeros(Hc.shape[:-2], dtype=np.int32)
        _check(self.lib, self.lib.tmpc_tracking_reference_host(self._h, ns, _dptr(Hc), _dptr(q), _dptr(wref), float(ts), _dptr(W), _dptr(yref),
                                                              info.ctypes.data_as(C.POINTER(C.c_int32))), 'tmpc_tracking_reference_host')
        return W, yref, info

    def debug_factor_bench(self, nb, p, d, reps=3):
        """(factorisation ms, single-rhs solve ms) of nb copies of one random SPD block-cyclic-tridiagonal system."""
        out = np.zeros(2)
        _check(self.lib, self.lib.tmpc_debug_factor_bench(self._h, nb, p, d, reps, _dptr(out)), 'tmpc_debug_factor_bench')
        return out

    def debug_last_trsm_pairs(self):
        """Two-edge items of k_cr_trsm_dma_f32 in the last debug_block_factor / debug_factor_bench (tmpc_debug_last_trsm_pairs: a host-side count)."""
        return int(self.lib.tmpc_debug_last_trsm_pairs())

    def debug_block_solve(self, D, Ccpl, rhs):
        D = np.ascontiguousarray(D, dtype=np.float64); Ccpl = np.ascontiguousarray(Ccpl, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        p, d, _ = D.shape
        x = np.empty((p, d)); ns = np.zeros(1, np.int32)
        _check(self.lib, self.lib.tmpc_debug_block_solve(self._h, p, d, _dptr(D), _dptr(Ccpl), _dptr(rhs), _dptr(x), _iptr(ns)), 'tmpc_debug_block_solve')
        return x, int(ns[0])

    def debug_block_factor(self, D, Ccpl, rhs, plist=None, lowp=None, pass1=False, fuse_fwd1=False, lowp_trsm=False, dd=False, Dlo=None, Clo=None):
        """tmpc_debug_block_factor: the block factorisation and its substitutions as the solver drives them, on nb distinct systems
        D, Ccpl [nb, p, d, d], rhs [nb, p, d] (pass 2) or [nb, p, d, 3] (pass1=True), for the problems of `plist` (ordered subset of range(nb); default all),
        lowp [nb]: 1 = float32 updates for that problem, lowp_trsm: their solves in float32 too; dd: in double-double (Dlo / Clo: low words).
        Returns, for EVERY problem of the batch: L [nb, p, d, d] (lower triangle of D after the call), D, O, F (un-padded block arrays; O, F in the slot
        orientation `orient`), O32 [nb, 2p, d, d] or None, Ddiag, x, the low words Dl / Ol / Fl / xl (dd), nshift [nb], and under 'raw' the padded device
        images with dp, ld32."""
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        D, Ccpl, rhs, Dlo, Clo = f64(D), f64(Ccpl), f64(rhs), f64(Dlo), f64(Clo)
        nb, p, d, _ = D.shape
        nc = 3 if pass1 else 1
        if Ccpl.shape != D.shape or rhs.shape != ((nb, p, d, 3) if pass1 else (nb, p, d)):
            raise ValueError('debug_block_factor: D, Ccpl [nb, p, d, d] and rhs [nb, p, d] (pass 2) / [nb, p, d, 3] (pass 1) expected')
        plist = np.ascontiguousarray(np.arange(nb) if plist is None else plist, dtype=np.int32)
        lowp = None if lowp is None else np.ascontiguousarray(lowp, dtype=np.int32)
        if lowp is not None and lowp.shape != (nb,):
            raise ValueError('debug_block_factor: lowp [nb] expected')
        mode = (FACTOR_PASS1 if pass1 else 0) | (FACTOR_FUSE_FWD1 if fuse_fwd1 else 0) | (FACTOR_LOWP_TRSM if lowp_trsm else 0) | (FACTOR_DD if dd else 0)
        dp = (d + 15) // 16 * 16; ld32 = (dp + 31) // 32 * 32
        has32 = bool(lowp_trsm or (lowp is not None and lowp.any()))
        raw = dict(D=np.empty((nb, p, dp, dp)), O=np.empty((nb, p, dp, dp)), F=np.empty((nb, p, dp, dp)), Ddiag=np.empty((nb, p, dp)), X=np.empty((nb, p, dp, nc)),
                   O32=np.empty((nb, 2 * p, dp, ld32), np.float32) if has32 else None)
        if dd:
            raw.update(Dl=np.empty((nb, p, dp, dp)), Ol=np.empty((nb, p, dp, dp)), Fl=np.empty((nb, p, dp, dp)), Xl=np.empty((nb, p, dp, nc)))
        nshift = np.zeros(nb, np.int32); dims = np.zeros(4, np.int32); orient = np.zeros(p, np.int32)
        io = _FactorIO(D=_dptr(D), Ccpl=_dptr(Ccpl), Dlo=_dptr(Dlo), Clo=_dptr(Clo), rhs=_dptr(rhs), list=_iptr(plist), lowp=_iptr(lowp),
                       oD=_dptr(raw['D']), oO=_dptr(raw['O']), oF=_dptr(raw['F']), oDdiag=_dptr(raw['Ddiag']), oX=_dptr(raw['X']),
                       oO32=raw['O32'].ctypes.data_as(C.POINTER(C.c_float)) if has32 else None,
                       oDl=_dptr(raw.get('Dl')), oOl=_dptr(raw.get('Ol')), oFl=_dptr(raw.get('Fl')), oXl=_dptr(raw.get('Xl')),
                       nshift=_iptr(nshift), dims=_iptr(dims), orient=_iptr(orient))
        _check(self.lib, self.lib.tmpc_debug_block_factor(self._h, nb, p, d, len(plist), mode, C.byref(io)), 'tmpc_debug_block_factor')
        assert (int(dims[0]), int(dims[1]), int(dims[2]), bool(dims[3])) == (dp, ld32, nc, has32), dims
        raw.update(dp=dp, ld32=ld32)
        cut = lambda a: None if a is None else a[:, :, :d, :d].copy()
        vec = lambda a: None if a is None else (a[:, :, :d, :].copy() if pass1 else a[:, :, :d, 0].copy())
        out = dict(raw=raw, orient=orient, nshift=nshift, D=cut(raw['D']), L=np.tril(cut(raw['D'])), O=cut(raw['O']), F=cut(raw['F']), O32=cut(raw['O32']),
                   Ddiag=raw['Ddiag'][:, :, :d].copy(), x=vec(raw['X']))
        if dd:
            out.update(Dl=cut(raw['Dl']), Ll=np.tril(cut(raw['Dl'])), Ol=cut(raw['Ol']), Fl=cut(raw['Fl']), xl=vec(raw['Xl']))
        return out


def eig_clip(A, tol):
    """out = sym(A) + V diag(max(tol - lambda, 0)) V' for one (n x n) or a batch ([nb, n, n]) of symmetric matrices, any n
    (tmpc_eig_clip_host; reference sqp_method.py:327-403).  Returns dict(out, evals, reg, sweeps)."""
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float64)
    single = A.ndim == 2
    A3 = A[None] if single else A
    nb, n, n2 = A3.shape
    if n != n2:
        raise ValueError('square matrices expected')
    out = np.empty_like(A3); ev = np.empty((nb, n)); reg = np.empty(nb); sw = np.zeros(nb, dtype=np.int32)
    rc = lib.tmpc_eig_clip_host(nb, n, _dptr(A3), float(tol), _dptr(out), _dptr(ev), _dptr(reg), _iptr(sw))
    if rc == E_NOCONV:
        err = EigNotConverged(f"tunempc_amd: tmpc_eig_clip_host did not converge: {lib.tmpc_last_error().decode()}")
        err.partial = dict(out=out, evals=ev, reg=reg, sweeps=sw)
        raise err
    _check(lib, rc, 'tmpc_eig_clip_host')
    if single:
        return dict(out=out[0], evals=ev[0], reg=float(reg[0]), sweeps=int(sw[0]))
    return dict(out=out, evals=ev, reg=reg, sweeps=sw)


def _check_lqr(lib, rc, what):
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(lib.tmpc_last_error().decode())
    _check(lib, rc, what)


def periodic_lqr_batch_host(A, B, H, Pi0, tol, max_sweeps):
    """tmpc_periodic_lqr_batch_host on validated, contiguous fp64 numpy arrays -> (K, Pi, Phi, info)."""
    lib = load_library()
    nb, p, nx, mb = B.shape
    K = np.empty((nb, p, mb, nx)); Pi = np.empty((nb, p, nx, nx)); Phi = np.empty((nb, nx, nx)); info = np.zeros((nb, LQR_INFO_STRIDE))
    rc = lib.tmpc_periodic_lqr_batch_host(nb, p, nx, mb, _dptr(A), _dptr(B), _dptr(H), _dptr(Pi0), float(tol), int(max_sweeps),
                                          _dptr(K), _dptr(Pi), _dptr(Phi), _dptr(info))
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_batch_host')
    return K, Pi, Phi, info


def periodic_lqr_batch_device(A, B, H, Pi0, tol, max_sweeps):
    """tmpc_periodic_lqr_batch_device on validated, contiguous fp64 torch tensors of one GPU -> (K, Pi, Phi, info) tensors; A / B / H never leave HBM."""
    import torch
    lib = load_library()
    nb, p, nx, mb = B.shape
    dev = A.device
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    K, Pi, Phi, info = f64(nb, p, mb, nx), f64(nb, p, nx, nx), f64(nb, nx, nx), torch.zeros((nb, LQR_INFO_STRIDE), dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
        rc = lib.tmpc_periodic_lqr_batch_device(nb, p, nx, mb, ptr(A), ptr(B), ptr(H), ptr(Pi0), float(tol), int(max_sweeps),
                                                ptr(K), ptr(Pi), ptr(Phi), ptr(info))
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_batch_device')
    return K, Pi, Phi, info


def periodic_lqr_rows_batch_host(A, B, H, J, ncnt, ng, Pi0, tol, max_sweeps):
    """tmpc_periodic_lqr_rows_batch_host on validated, contiguous numpy arrays (fp64; ncnt int32 or None) -> (K, Pi, Phi, Lam, info)."""
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = J.shape[2]
    K = np.empty((nb, p, mb, nx)); Pi = np.empty((nb, p, nx, nx)); Phi = np.empty((nb, nx, nx)); Lam = np.zeros((nb, p, nr, nx))
    info = np.zeros((nb, LQR_INFO_STRIDE))
    rc = lib.tmpc_periodic_lqr_rows_batch_host(nb, p, nx, mb, nr, int(ng), _dptr(A), _dptr(B), _dptr(H), _dptr(J), _iptr(ncnt), _dptr(Pi0), float(tol),
                                               int(max_sweeps), _dptr(K), _dptr(Pi), _dptr(Phi), _dptr(Lam), _dptr(info))
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_rows_batch_host')
    return K, Pi, Phi, Lam, info


def periodic_lqr_rows_batch_device(A, B, H, J, ncnt, ng, Pi0, tol, max_sweeps):
    """tmpc_periodic_lqr_rows_batch_device on validated, contiguous torch tensors of one GPU (fp64; ncnt int32 or None) -> (K, Pi, Phi, Lam, info) tensors;
    A / B / H / J never leave HBM."""
    import torch
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = J.shape[2]
    dev = A.device
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    K, Pi, Phi, info = f64(nb, p, mb, nx), f64(nb, p, nx, nx), f64(nb, nx, nx), torch.zeros((nb, LQR_INFO_STRIDE), dtype=torch.float64, device=dev)
    Lam = torch.zeros((nb, p, nr, nx), dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
        rc = lib.tmpc_periodic_lqr_rows_batch_device(nb, p, nx, mb, nr, int(ng), ptr(A), ptr(B), ptr(H), ptr(J), ptr(ncnt), ptr(Pi0), float(tol),
                                                     int(max_sweeps), ptr(K), ptr(Pi), ptr(Phi), ptr(Lam), ptr(info))
    if rc == -1:
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_rows_batch_device')
    return K, Pi, Phi, Lam, info


def periodic_lqr_ctg_batch_host(A, B, H, J, ncnt, ng, Pi0, tol, rank_tol, max_sweeps):
    """tmpc_periodic_lqr_ctg_batch_host on validated, contiguous numpy arrays (fp64; ncnt int32 or None) -> (K, Pi, Phi, Hn, cnt, info)."""
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = J.shape[2]
    K = np.empty((nb, p, mb, nx)); Pi = np.empty((nb, p, nx, nx)); Phi = np.empty((nb, nx, nx)); Hn = np.zeros((nb, p, nx, nx))
    cnt = np.zeros((nb, p), np.int32); info = np.zeros((nb, LQR_CTG_INFO_STRIDE))
    rc = lib.tmpc_periodic_lqr_ctg_batch_host(nb, p, nx, mb, nr, int(ng), _dptr(A), _dptr(B), _dptr(H), _dptr(J), _iptr(ncnt), _dptr(Pi0), float(tol),
                                              float(rank_tol), int(max_sweeps), _dptr(K), _dptr(Pi), _dptr(Phi), _dptr(Hn), _iptr(cnt), _dptr(info))
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_ctg_batch_host')
    return K, Pi, Phi, Hn, cnt, info


def periodic_lqr_ctg_batch_device(A, B, H, J, ncnt, ng, Pi0, tol, rank_tol, max_sweeps):
    """tmpc_periodic_lqr_ctg_batch_device on validated, contiguous torch tensors of one GPU (fp64; ncnt int32 or None) -> (K, Pi, Phi, Hn, cnt, info)
    tensors; A / B / H / J never leave HBM."""
    import torch
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = J.shape[2]
    dev = A.device
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    K, Pi, Phi, info = f64(nb, p, mb, nx), f64(nb, p, nx, nx), f64(nb, nx, nx), torch.zeros((nb, LQR_CTG_INFO_STRIDE), dtype=torch.float64, device=dev)
    Hn = torch.zeros((nb, p, nx, nx), dtype=torch.float64, device=dev); cnt = torch.zeros((nb, p), dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
        rc = lib.tmpc_periodic_lqr_ctg_batch_device(nb, p, nx, mb, nr, int(ng), ptr(A), ptr(B), ptr(H), ptr(J), ptr(ncnt), ptr(Pi0), float(tol),
                                                    float(rank_tol), int(max_sweeps), ptr(K), ptr(Pi), ptr(Phi), ptr(Hn), ptr(cnt), ptr(info))
    if rc == -1:
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_periodic_lqr_ctg_batch_device')
    return K, Pi, Phi, Hn, cnt, info


def horizon_lqr_batch_host(A, B, H, J, ncnt, ng, N, phases, terminal, Pf, rank_tol, return_all):
    """tmpc_horizon_lqr_batch_host on validated, contiguous numpy arrays (fp64; J None or [nb,p,nr,n]; ncnt int32 or None; phases int32 [nph] or None: all p;
    terminal 0 cost / 1 constraint) -> (K0, Pi0, Hn0, cnt0, Kall or None, cntall or None, info)."""
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = 0 if J is None else J.shape[2]
    nph = p if phases is None else len(phases)
    K0 = np.empty((nb, nph, mb, nx)); Pi0 = np.empty((nb, nph, nx, nx)); Hn0 = np.zeros((nb, nph, nx, nx)); cnt0 = np.zeros((nb, nph), np.int32)
    info = np.zeros((nb, nph, LQR_CTG_INFO_STRIDE))
    Kall = np.empty((nb, nph, int(N), mb, nx)) if return_all else None
    cntall = np.zeros((nb, nph, int(N)), np.int32) if return_all else None
    rc = lib.tmpc_horizon_lqr_batch_host(nb, p, nx, mb, nr, int(ng), int(N), nph, _iptr(phases), int(terminal), _dptr(A), _dptr(B), _dptr(H),
                                         _dptr(J) if nr else None, _iptr(ncnt), _dptr(Pf), float(rank_tol), _dptr(K0), _dptr(Pi0), _dptr(Hn0), _iptr(cnt0),
                                         _dptr(Kall), _iptr(cntall), _dptr(info))
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_horizon_lqr_batch_host')
    return K0, Pi0, Hn0, cnt0, Kall, cntall, info


def horizon_lqr_batch_device(A, B, H, J, ncnt, ng, N, phases, terminal, Pf, rank_tol, return_all):
    """tmpc_horizon_lqr_batch_device on validated, contiguous torch tensors of one GPU (fp64; ncnt int32 or None); phases is a numpy int32 array or None (the
    entry takes the list from the host) -> (K0, Pi0, Hn0, cnt0, Kall or None, cntall or None, info) tensors; A / B / H / J / Pf never leave HBM."""
    import torch
    lib = load_library()
    nb, p, nx, mb = B.shape
    nr = 0 if J is None else J.shape[2]
    nph = p if phases is None else len(phases)
    dev = A.device
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    K0, Pi0, info = f64(nb, nph, mb, nx), f64(nb, nph, nx, nx), torch.zeros((nb, nph, LQR_CTG_INFO_STRIDE), dtype=torch.float64, device=dev)
    Hn0 = torch.zeros((nb, nph, nx, nx), dtype=torch.float64, device=dev); cnt0 = torch.zeros((nb, nph), dtype=torch.int32, device=dev)
    Kall = f64(nb, nph, int(N), mb, nx) if return_all else None
    cntall = torch.zeros((nb, nph, int(N)), dtype=torch.int32, device=dev) if return_all else None
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
        rc = lib.tmpc_horizon_lqr_batch_device(nb, p, nx, mb, nr, int(ng), int(N), nph, _iptr(phases), int(terminal), ptr(A), ptr(B), ptr(H), ptr(J), ptr(ncnt),
                                               ptr(Pf), float(rank_tol), ptr(K0), ptr(Pi0), ptr(Hn0), ptr(cnt0), ptr(Kall), ptr(cntall), ptr(info))
    if rc == -1:
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_horizon_lqr_batch_device')
    return K0, Pi0, Hn0, cnt0, Kall, cntall, info


def _closed_loop_views(X, U, l, lc, rowres, subres, sums, XT, info, tr4, tr3):
    """The outputs of the closed-loop entries (time-major in memory) in the layout of closed_loop_batch: permuted views, nothing is copied."""
    return dict(X=None if X is None else tr4(X), U=None if U is None else tr4(U), l=None if l is None else tr3(l), lc=None if lc is None else tr3(lc),
                rowres=None if rowres is None else tr3(rowres), subres=None if subres is None else tr3(subres), sums=sums, XT=XT, info=info)


def closed_loop_batch_host(A, B, K, X0, H, Hc, J, ncnt, ng, Hn, T, k0, return_traj):
    """tmpc_closed_loop_batch_host on validated, contiguous numpy arrays (fp64; H, Hc, J, Hn None or arrays; ncnt int32 or None) -> dict X [nb,ns,T+1,nx],
    U [nb,ns,T,nu] (None without return_traj), l, lc, rowres, subres [nb,ns,T] (None without their input), sums [nb,ns,2] (None without a cost), XT [nb,ns,nx],
    info [nb,ns,4].  The library stores the trajectories time-major: X, U and the per-step scalars are permuted views of those arrays."""
    lib = load_library()
    nb, p, nx, mb = B.shape
    ns, T = X0.shape[1], int(T)
    nr = 0 if J is None else J.shape[2]
    X = np.empty((nb, T + 1, ns, nx)) if return_traj else None
    U = np.empty((nb, T, ns, mb)) if return_traj else None
    step = lambda have: np.empty((nb, T, ns)) if have is not None else None
    l, lc, rowres, subres = step(H), step(Hc), step(J if nr else None), step(Hn)
    sums = np.empty((nb, ns, 2)) if (H is not None or Hc is not None) else None
    XT = np.empty((nb, ns, nx)); info = np.zeros((nb, ns, CLOSED_LOOP_INFO_STRIDE))
    rc = lib.tmpc_closed_loop_batch_host(nb, p, nx, mb, nr, int(ng), ns, T, int(k0), _dptr(A), _dptr(B), _dptr(K), _dptr(X0), _dptr(H), _dptr(Hc),
                                         _dptr(J) if nr else None, _iptr(ncnt) if nr else None, _dptr(Hn), _dptr(X), _dptr(U), _dptr(l), _dptr(lc), _dptr(rowres),
                                         _dptr(subres), _dptr(sums), _dptr(XT), _dptr(info))
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_closed_loop_batch_host')
    return _closed_loop_views(X, U, l, lc, rowres, subres, sums, XT, info, lambda a: a.transpose(0, 2, 1, 3), lambda a: a.transpose(0, 2, 1))


def closed_loop_batch_device(A, B, K, X0, H, Hc, J, ncnt, ng, Hn, T, k0, return_traj):
    """tmpc_closed_loop_batch_device on validated, contiguous torch tensors of one GPU (fp64; ncnt int32 or None) -> the dict of closed_loop_batch_host with
    torch tensors; the inputs never leave HBM."""
    import torch
    lib = load_library()
    nb, p, nx, mb = B.shape
    ns, T = X0.shape[1], int(T)
    nr = 0 if J is None else J.shape[2]
    dev = A.device
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    X = f64(nb, T + 1, ns, nx) if return_traj else None
    U = f64(nb, T, ns, mb) if return_traj else None
    step = lambda have: f64(nb, T, ns) if have is not None else None
    l, lc, rowres, subres = step(H), step(Hc), step(J if nr else None), step(Hn)
    sums = f64(nb, ns, 2) if (H is not None or Hc is not None) else None
    XT = f64(nb, ns, nx); info = torch.zeros((nb, ns, CLOSED_LOOP_INFO_STRIDE), dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
        rc = lib.tmpc_closed_loop_batch_device(nb, p, nx, mb, nr, int(ng), ns, T, int(k0), ptr(A), ptr(B), ptr(K), ptr(X0), ptr(H), ptr(Hc), ptr(J) if nr else None,
                                               ptr(ncnt) if nr else None, ptr(Hn), ptr(X), ptr(U), ptr(l), ptr(lc), ptr(rowres), ptr(subres), ptr(sums), ptr(XT),
                                               ptr(info))
    if rc == -1:
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, 'tmpc_closed_loop_batch_device')
    return _closed_loop_views(X, U, l, lc, rowres, subres, sums, XT, info, lambda a: a.permute(0, 2, 1, 3), lambda a: a.permute(0, 2, 1))


class _HostArrays:
    """The array kind of the host entries for _mpc_qp_call: numpy allocation, the pointer of an optional array, the axis permutation, the call."""
    entry = 'host'

    def __init__(self, like):
        pass

    def f64(self, *sh):
        return np.empty(sh)

    def i32(self, *sh):
        return np.empty(sh, np.int32)

    def zeros(self, *sh):
        return np.zeros(sh)

    @staticmethod
    def ptr(a):
        if a is None or not a.size:
            return None
        return _iptr(a) if a.dtype == np.int32 else _dptr(a)

    @staticmethod
    def permute(a, *axes):
        return a.transpose(*axes)

    def call(self, fn, args):
        return fn(*args)


class _DeviceArrays:
    """The same for the device entries: torch tensors on the GPU of `like`."""
    entry = 'device'

    def __init__(self, like):
        import torch
        self.torch, self.dev = torch, like.device

    def f64(self, *sh):
        return self.torch.empty(sh, dtype=self.torch.float64, device=self.dev)

    def i32(self, *sh):
        return self.torch.empty(sh, dtype=self.torch.int32, device=self.dev)

    def zeros(self, *sh):
        return self.torch.zeros(sh, dtype=self.torch.float64, device=self.dev)

    @staticmethod
    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    @staticmethod
    def permute(t, *axes):
        return t.permute(*axes)

    def call(self, fn, args):
        with self.torch.cuda.device(self.dev):
            self.torch.cuda.current_stream(self.dev).synchronize()      # the entry runs on the null stream: the inputs must be complete
            return fn(*args)


def _mpc_qp_eq_terminal(Tx, nx):
    """Tx None / 'constraint' / array [nb,p,nt,nx] -> (nt argument of the C entry, array or None, rows of NuT)."""
    if Tx is None:
        return 0, None, 0
    if isinstance(Tx, str):
        return -1, None, nx
    return int(Tx.shape[2]), Tx, int(Tx.shape[2])


_MPC_QP_LEVELS = {'hard': '', 'soft': 'soft_', 'eq': 'eq_', 'aff': 'aff_', 'quad': 'quad_', 'warm': 'warm_'}


def _mpc_qp_call(level, kind, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty=None, J=None, r=None, necnt=None,
                 Tx=None, aff=None, penalty2=None, warm=None):
    """The twelve MPC QP entries: tmpc_mpc_qp_<level>batch_<host or device> of the level 'hard', 'soft', 'eq', 'aff', 'quad' or 'warm' on validated, contiguous arrays of `kind`
    (_HostArrays: numpy, _DeviceArrays: torch tensors of one GPU).  Allocates the outputs, passes the 31 common arguments and the tails of the level (soft:
    penalty, Eol, nviol; eq: the rows and Nu, NuT, eres; aff: the seven arrays; quad: penalty2; warm = (flags, floor, Xg, Ug, Lamg, Eg, Nug, NuTg): these and
    warmlog), an absent or empty array as NULL, and returns the dict of the level (warm: with warmlog [nb,ns,T] int32).  The
    library stores the logs time-major: X, U and the per-step logs are permuted views, nothing is copied."""
    lib = load_library()
    xp = kind(A)
    name = 'tmpc_mpc_qp_%sbatch_%s' % (_MPC_QP_LEVELS[level], xp.entry)
    nb, p, nx, mb = B.shape
    ns, T, N = X0.shape[1], int(T), int(N)
    nd = 0 if D is None else D.shape[2]
    ne = 0 if J is None else J.shape[2]
    nt, Txa, ntr = _mpc_qp_eq_terminal(Tx, nx)
    eq = level in ('eq', 'aff', 'quad', 'warm')
    soft = level == 'soft' or (eq and penalty is not None)                  # (the eq level without penalty passes Eol = nviol = NULL)
    traj = lambda *sh: xp.f64(*sh) if return_traj else None
    ol = lambda *sh: xp.f64(*sh) if return_ol else None
    X, U = traj(nb, T + 1, ns, nx), traj(nb, T, ns, mb)
    iters, nact, hres = xp.i32(nb, T, ns), xp.i32(nb, T, ns), xp.f64(nb, T, ns)
    Xol, Uol, Lam = ol(nb, ns, N + 1, nx), ol(nb, ns, N, mb), ol(nb, ns, N, nd)
    U0, XT, info = xp.f64(nb, ns, mb), xp.f64(nb, ns, nx), xp.zeros(nb, ns, MPC_QP_INFO_STRIDE)
    Eol, nviol = (ol(nb, ns, N, nd), xp.i32(nb, T, ns)) if soft else (None, None)
    Nu, NuT, eres = (ol(nb, ns, N, ne), ol(nb, ns, ntr), xp.f64(nb, T, ns)) if eq else (None, None, None)
    ptr = xp.ptr
    rows = lambda a, cap: ptr(a) if cap else None
    args = [nb, p, nx, mb, nd, N, ns, T, int(k0), ptr(A), ptr(B), ptr(H), ptr(q), ptr(Pf), rows(D, nd), rows(ndcnt, nd), rows(d, nd), ptr(X0), float(tol),
            int(max_iter)] + [ptr(a) for a in (U0, XT, info, X, U, iters, nact, hres, Xol, Uol, Lam)]
    if level != 'hard':
        args += [ptr(penalty), ptr(Eol), ptr(nviol)]
    if eq:
        args += [ne, rows(J, ne), rows(r, ne), rows(necnt, ne), nt, ptr(Txa), ptr(Nu), ptr(NuT), ptr(eres)]
    if level in ('aff', 'quad', 'warm'):
        args += [ptr(a) for a in (aff if aff is not None else (None,) * 7)]
    if level in ('quad', 'warm'):
        args += [ptr(penalty2)]
    if level == 'warm':
        warmlog = xp.i32(nb, T, ns)
        args += [int(warm[0]), float(warm[1])] + [None if a is None else ptr(a) for a in warm[2:8]] + [ptr(warmlog)]
    rc = xp.call(getattr(lib, name), args)
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, name)
    tr4, tr3 = (lambda a: None if a is None else xp.permute(a, 0, 2, 1, 3)), (lambda a: xp.permute(a, 0, 2, 1))
    out = dict(U0=U0, XT=XT, info=info, X=tr4(X), U=tr4(U), iters=tr3(iters), nact=tr3(nact), hres=tr3(hres), Xol=Xol, Uol=Uol, Lam=Lam)
    if eq:
        out.update(Nu=Nu, NuT=NuT, eres=tr3(eres))
    if soft:
        out.update(Eol=Eol, nviol=tr3(nviol))
    if level == 'warm':
        out['warmlog'] = tr3(warmlog)
    return out


def mpc_qp_batch_host(A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_batch_host on validated, contiguous numpy arrays (fp64; q, Pf, D, d None or arrays; ndcnt int32 or None) -> dict U0 [nb,ns,nu], XT [nb,ns,nx],
    info [nb,ns,8], X [nb,ns,T+1,nx], U [nb,ns,T,nu] (None without return_traj), iters, nact int32 [nb,ns,T], hres [nb,ns,T], Xol [nb,ns,N+1,nx], Uol [nb,ns,N,nu],
    Lam [nb,ns,N,nd] (None without return_ol)."""
    return _mpc_qp_call('hard', _HostArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol)


def mpc_qp_batch_device(A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_batch_device on validated, contiguous torch tensors of one GPU (fp64; ndcnt int32 or None) -> the dict of mpc_qp_batch_host with torch
    tensors; the inputs never leave HBM."""
    return _mpc_qp_call('hard', _DeviceArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol)


def mpc_qp_soft_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_soft_batch_host on validated, contiguous numpy arrays (penalty fp64 [nb,p,nd]) -> the dict of mpc_qp_batch_host with Eol [nb,ns,N,nd] (None
    without return_ol) and nviol int32 [nb,ns,T]."""
    return _mpc_qp_call('soft', _HostArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty)


def mpc_qp_soft_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_soft_batch_device on validated, contiguous torch tensors of one GPU -> the dict of mpc_qp_soft_batch_host with torch tensors."""
    return _mpc_qp_call('soft', _DeviceArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty)


def mpc_qp_eq_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, X0, N, T, k0, tol, max_iter, return_traj, return_ol, aff=None):
    """tmpc_mpc_qp_eq_batch_host on validated, contiguous numpy arrays (penalty, J [nb,p,ne,n], r, necnt int32 None or arrays; Tx None, 'constraint' or
    [nb,p,nt,nx]) -> the dict of mpc_qp_soft_batch_host (Eol None and no nviol without penalty) with Nu [nb,ns,N,ne], NuT [nb,ns,nt] (None without return_ol)
    and eres [nb,ns,T].  aff (mpc_qp_aff_batch_host): the seven arrays offset, qf, terminal_rhs, Ap, Bp, cp, W or None each -> tmpc_mpc_qp_aff_batch_host."""
    return _mpc_qp_call('eq' if aff is None else 'aff', _HostArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty, J,
                        r, necnt, Tx, aff)


def mpc_qp_eq_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, X0, N, T, k0, tol, max_iter, return_traj, return_ol, aff=None):
    """tmpc_mpc_qp_eq_batch_device on validated, contiguous torch tensors of one GPU -> the dict of mpc_qp_eq_batch_host with torch tensors.  aff as there:
    tmpc_mpc_qp_aff_batch_device."""
    return _mpc_qp_call('eq' if aff is None else 'aff', _DeviceArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty,
                        J, r, necnt, Tx, aff)


def mpc_qp_aff_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_aff_batch_host on validated, contiguous numpy arrays: the arguments of mpc_qp_eq_batch_host and aff = (offset, qf, terminal_rhs, Ap, Bp, cp,
    W), None or an array each -> the dict of mpc_qp_eq_batch_host."""
    return mpc_qp_eq_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, X0, N, T, k0, tol, max_iter, return_traj, return_ol, aff=tuple(aff))


def mpc_qp_aff_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_aff_batch_device on validated, contiguous torch tensors of one GPU -> the dict of mpc_qp_aff_batch_host with torch tensors."""
    return mpc_qp_eq_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, X0, N, T, k0, tol, max_iter, return_traj, return_ol, aff=tuple(aff))


def cr_schedule(p):
    """The elimination schedule of the block factorisation for period p (host only): dict(prep, levels [(eoff, nelim, uoff, nupd)],
    elim [nelim, 8], upd [nupd, 8], orient [p]) -- see include/tunempc_hip_debug.h."""
    lib = load_library()
    n = lib.tmpc_debug_cr_schedule(int(p), None, 0)
    if n < 0:
        raise ValueError('cr_schedule: p >= 1 expected')
    buf = np.zeros(n, np.int32)
    lib.tmpc_debug_cr_schedule(int(p), _iptr(buf), n)
    nlev, prep, ne, nu = (int(v) for v in buf[:4])
    o = 4
    levels = buf[o:o + 4 * nlev].reshape(nlev, 4); o += 4 * nlev
    elim = buf[o:o + 8 * ne].reshape(ne, 8); o += 8 * ne
    upd = buf[o:o + 8 * nu].reshape(nu, 8); o += 8 * nu
    return dict(prep=prep, levels=levels, elim=elim, upd=upd, orient=buf[o:o + p].copy())


def mpc_qp_quad_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, penalty2, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_quad_batch_host on validated, contiguous numpy arrays: the arguments of mpc_qp_aff_batch_host (aff None: no affine array) and penalty2
    [nb,p,nd] -> the dict of mpc_qp_eq_batch_host (Eol: lam / Z on the pure quadratic rows)."""
    return _mpc_qp_call('quad', _HostArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty, J, r, necnt, Tx,
                        None if aff is None else tuple(aff), penalty2)


def mpc_qp_quad_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, penalty2, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_quad_batch_device on validated, contiguous torch tensors of one GPU -> the dict of mpc_qp_quad_batch_host with torch tensors."""
    return _mpc_qp_call('quad', _DeviceArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty, J, r, necnt, Tx,
                        None if aff is None else tuple(aff), penalty2)


def mpc_qp_warm_batch_host(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, penalty2, warm, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_warm_batch_host on validated, contiguous numpy arrays: the arguments of mpc_qp_quad_batch_host (penalty, penalty2, aff None where the call
    has none) and warm = (flags, floor, Xg, Ug, Lamg, Eg, Nug, NuTg), the guess arrays None or arrays -> the dict of mpc_qp_eq_batch_host with warmlog
    [nb,ns,T] int32 (0 cold, 1 warm, 2 the cold restart of a failed warm attempt, -1 from a failed step on)."""
    return _mpc_qp_call('warm', _HostArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty, J, r, necnt, Tx,
                        None if aff is None else tuple(aff), penalty2, tuple(warm))


def mpc_qp_warm_batch_device(A, B, H, q, Pf, D, ndcnt, d, penalty, J, r, necnt, Tx, aff, penalty2, warm, X0, N, T, k0, tol, max_iter, return_traj, return_ol):
    """tmpc_mpc_qp_warm_batch_device on validated, contiguous torch tensors of one GPU -> the dict of mpc_qp_warm_batch_host with torch tensors."""
    return _mpc_qp_call('warm', _DeviceArrays, A, B, H, q, Pf, D, ndcnt, d, X0, N, T, k0, tol, max_iter, return_traj, return_ol, penalty, J, r, necnt, Tx,
                        None if aff is None else tuple(aff), penalty2, tuple(warm))


def _mpc_qp_gain_call(kind, A, B, H, Pf, D, ndcnt, d, penalty, penalty2, J, necnt, terminal, Tx, X, U, Lam, Eps, cls_in, N, k0, rank_tol, return_all):
    """tmpc_mpc_qp_gain_batch_<host or device> on validated, contiguous arrays of `kind` (_HostArrays: numpy, _DeviceArrays: torch tensors of one GPU; fp64,
    the counts and cls_in int32; an absent or empty array is passed as NULL; terminal 0 none / 1 x_N = 0 / 2 the rows Tx) -> dict K0 [nb,ns,nu,nx], Pi0, Hn0
    [nb,ns,nx,nx], cnt0 int32 [nb,ns], info [nb,ns,12], cls int32 [nb,ns,N,nd], strict [nb,ns]; with return_all Kall [nb,ns,N,nu,nx], cntall int32 [nb,ns,N],
    dX [nb,ns,N+1,nx,nx], dU [nb,ns,N,nu,nx]."""
    lib = load_library()
    xp = kind(A)
    name = 'tmpc_mpc_qp_gain_batch_%s' % xp.entry
    nb, p, nx, mb = B.shape
    ns, N = X.shape[1], int(N)
    nd = 0 if D is None else D.shape[2]
    ne = 0 if J is None else J.shape[2]
    nt = 0 if Tx is None else Tx.shape[2]
    K0, Pi0, Hn0, cnt0, info = xp.f64(nb, ns, mb, nx), xp.f64(nb, ns, nx, nx), xp.f64(nb, ns, nx, nx), xp.i32(nb, ns), xp.zeros(nb, ns, LQR_CTG_INFO_STRIDE)
    cls, strict = xp.i32(nb, ns, N, nd), xp.f64(nb, ns)
    Kall, cntall, dX, dU = (xp.f64(nb, ns, N, mb, nx), xp.i32(nb, ns, N), xp.f64(nb, ns, N + 1, nx, nx), xp.f64(nb, ns, N, mb, nx)) if return_all else (None,) * 4
    ptr = xp.ptr
    rows = lambda a, cap: ptr(a) if cap else None
    args = [nb, p, nx, mb, nd, ne, nt, N, ns, int(k0), int(terminal), ptr(A), ptr(B), ptr(H), ptr(Pf), rows(D, nd), rows(ndcnt, nd), rows(d, nd), rows(penalty, nd),
            rows(penalty2, nd), rows(J, ne), rows(necnt, ne), ptr(Tx), ptr(X), ptr(U), rows(Lam, nd), rows(Eps, nd), rows(cls_in, nd), float(rank_tol)]
    args += [ptr(a) for a in (K0, Pi0, Hn0, cnt0, info, cls, strict, Kall, cntall, dX, dU)]
    rc = xp.call(getattr(lib, name), args)
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, name)
    out = dict(K0=K0, Pi0=Pi0, Hn0=Hn0, cnt0=cnt0, info=info, cls=cls, strict=strict)
    if return_all:
        out.update(Kall=Kall, cntall=cntall, dX=dX, dU=dU)
    return out


def mpc_qp_gain_batch_host(*args):
    """tmpc_mpc_qp_gain_batch_host on numpy arrays: _mpc_qp_gain_call."""
    return _mpc_qp_gain_call(_HostArrays, *args)


def mpc_qp_gain_batch_device(*args):
    """tmpc_mpc_qp_gain_batch_device on torch tensors of one GPU: _mpc_qp_gain_call; the inputs never leave HBM."""
    return _mpc_qp_gain_call(_DeviceArrays, *args)


def _periodic_qp_call(kind, A, B, H, q, offset, D, ndcnt, d, J, r, necnt, periods, tol, max_iter):
    """tmpc_periodic_qp_batch_<host or device> on validated, contiguous arrays of `kind` (_HostArrays: numpy, _DeviceArrays: torch tensors of one GPU; fp64, the
    counts int32; an absent array is passed as NULL) -> dict X [nb,N,nx], U [nb,N,nu], lam [nb,N,nd], nu [nb,N,ne], pi [nb,N,nx], info [nb,8], res [nb,4]."""
    lib = load_library()
    xp = kind(A)
    name = 'tmpc_periodic_qp_batch_%s' % xp.entry
    nb, p, nx, mb = B.shape
    nd = 0 if D is None else D.shape[2]
    ne = 0 if J is None else J.shape[2]
    N = int(periods) * p
    X, U, Lam, Nu, Pi = xp.f64(nb, N, nx), xp.f64(nb, N, mb), xp.f64(nb, N, nd), xp.f64(nb, N, ne), xp.f64(nb, N, nx)
    info, res = xp.zeros(nb, PERIODIC_QP_INFO_STRIDE), xp.zeros(nb, PERIODIC_QP_RES_STRIDE)
    ptr = xp.ptr
    args = [nb, p, nx, mb, nd, ne, int(periods)] + [ptr(a) for a in (A, B, H, q, offset, D, ndcnt, d, J, r, necnt)] + [float(tol), int(max_iter)]
    args += [ptr(a) for a in (X, U, Lam, Nu, Pi, info, res)]
    rc = xp.call(getattr(lib, name), args)
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, name)
    return dict(X=X, U=U, lam=Lam, nu=Nu, pi=Pi, info=info, res=res)


def periodic_qp_batch_host(*args):
    """tmpc_periodic_qp_batch_host on numpy arrays: _periodic_qp_call."""
    return _periodic_qp_call(_HostArrays, *args)


def periodic_qp_batch_device(*args):
    """tmpc_periodic_qp_batch_device on torch tensors of one GPU: _periodic_qp_call; the inputs never leave HBM."""
    return _periodic_qp_call(_DeviceArrays, *args)


def _periodic_qp_soft_call(kind, A, B, H, q, offset, D, ndcnt, d, penalty, penalty2, J, r, necnt, periods, tol, max_iter):
    """tmpc_periodic_qp_soft_batch_<host or device> on validated, contiguous arrays of `kind` (as _periodic_qp_call; penalty, penalty2 [nb,p,nd] or None) ->
    dict X, U, lam, eps [nb,N,nd], nu, pi, nviol int32 [nb], info [nb,8], res [nb,6]."""
    lib = load_library()
    xp = kind(A)
    name = 'tmpc_periodic_qp_soft_batch_%s' % xp.entry
    nb, p, nx, mb = B.shape
    nd = 0 if D is None else D.shape[2]
    ne = 0 if J is None else J.shape[2]
    N = int(periods) * p
    X, U, Lam, Eps, Nu, Pi = xp.f64(nb, N, nx), xp.f64(nb, N, mb), xp.f64(nb, N, nd), xp.f64(nb, N, nd), xp.f64(nb, N, ne), xp.f64(nb, N, nx)
    nviol, info, res = xp.i32(nb), xp.zeros(nb, PERIODIC_QP_INFO_STRIDE), xp.zeros(nb, PERIODIC_QP_SOFT_RES_STRIDE)
    ptr = xp.ptr
    args = [nb, p, nx, mb, nd, ne, int(periods)] + [ptr(a) for a in (A, B, H, q, offset, D, ndcnt, d, penalty, penalty2, J, r, necnt)]
    args += [float(tol), int(max_iter)] + [ptr(a) for a in (X, U, Lam, Eps, Nu, Pi, nviol, info, res)]
    rc = xp.call(getattr(lib, name), args)
    if rc == -1:      # TMPC_E_ARG: the library's message names the argument
        raise ValueError(lib.tmpc_last_error().decode())
    _check_lqr(lib, rc, name)
    return dict(X=X, U=U, lam=Lam, eps=Eps, nu=Nu, pi=Pi, nviol=nviol, info=info, res=res)


def periodic_qp_soft_batch_host(*args):
    """tmpc_periodic_qp_soft_batch_host on numpy arrays: _periodic_qp_soft_call."""
    return _periodic_qp_soft_call(_HostArrays, *args)


def periodic_qp_soft_batch_device(*args):
    """tmpc_periodic_qp_soft_batch_device on torch tensors of one GPU: _periodic_qp_soft_call; the inputs never leave HBM."""
    return _periodic_qp_soft_call(_DeviceArrays, *args)
