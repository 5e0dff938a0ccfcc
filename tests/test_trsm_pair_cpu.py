"""Host side of TMPC_TUNE_TRSM_PAIR (two edges per workgroup in the float32 triangular solves), without a device: the key the header publishes,
its place in HipConvexifier.set_tuning, and the call that reaches tmpc_set_tuning."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defs():
    src = open(os.path.join(ROOT, 'include', 'tunempc_hip.h')).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define\s+(TMPC_[A-Z0-9_]+)\s+(-?\d+)\b', src, flags=re.M)}


def test_header_defines_the_key():
    defs = _defs()
    assert defs['TMPC_TUNE_TRSM_PAIR'] == 10
    keys = [v for k, v in defs.items() if k.startswith('TMPC_TUNE_')]
    assert len(keys) == len(set(keys))          # no key number is used twice
    assert defs['TMPC_TUNE_LOWP_TRSM'] == 9     # (the keys before it keep their numbers)


def test_set_tuning_ends_with_trsm_pair():
    from tunempc_amd._lib import HipConvexifier
    params = inspect.signature(HipConvexifier.set_tuning).parameters
    assert list(params)[-1] == 'trsm_pair' and params['trsm_pair'].default is None
    assert list(params)[-2] == 'lowp_trsm'


class _RecordingLib:
    """stands in for the loaded library: records what set_tuning sends"""
    def __init__(self):
        self.calls = []

    def tmpc_set_tuning(self, h, key, value):
        self.calls.append((key, value))
        return 0


def test_set_tuning_sends_key_10():
    from tunempc_amd._lib import HipConvexifier
    hc = object.__new__(HipConvexifier)        # no device: the handle is a stub, only the path to tmpc_set_tuning is exercised
    hc.lib = _RecordingLib(); hc._h = C.c_void_p()
    hc.set_tuning(trsm_pair=0)
    hc.set_tuning(lowp_trsm=1, trsm_pair=1)
    hc.set_tuning()
    assert hc.lib.calls == [(10, 0.0), (9, 1.0), (10, 1.0)]
    hc._h = None                                # (nothing to destroy)


def test_library_takes_the_key_and_exports_the_getter():
    """the real library: a NULL handle is refused for key 10 as for every key (no device needed), and the host-side getter exists and answers without one"""
    import __graft_entry__ as g
    g.build()
    from tunempc_amd._lib import load_library, DEBUG_EXPORTS
    lib = load_library()
    assert lib.tmpc_set_tuning(None, _defs()['TMPC_TUNE_TRSM_PAIR'], 0.0) != 0
    assert 'tmpc_debug_last_trsm_pairs' in DEBUG_EXPORTS
    assert lib.tmpc_debug_last_trsm_pairs() >= 0
