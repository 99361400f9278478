"""ctypes binding of libaqua_segments.so (include/aqua_segments.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- per-segment episode statistics have no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_SEGMENTS_LIB", "libaqua_segments.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_WORLDS = 1 << 30
MAX_SEGMENTS = 4096
MAX_WINDOW = 1024
HEADER = 4                        # uint64 slots of header[]: seen, missed, stray, the ticket
COUNTS = 8                        # uint64 slots per segment: episodes, by code 1..3, steps of finished episodes, three unused

# every symbol include/aqua_segments.h declares (tests/test_segments_cpu.py checks the library exports them all)
SYMBOLS = ("aquaseg_version", "aquaseg_last_error", "aquaseg_account")


class AquaSegmentsError(RuntimeError):
    pass


_vp, _i64 = ctypes.c_void_p, ctypes.c_int64
_SIGNATURES = {
    "aquaseg_account": ([_vp, _vp, _vp, _vp, _i64, _vp,                       # log_ret, log_len, log_code, log_world, C, counts
                         _i64, _i64, _i64, _i64, _i64,                        # env_offset, N, seg, P, W
                         _vp, _vp, _vp, _vp, _vp,                             # header, seg_counts, hyper, eps_state, eps_out
                         _vp, _vp, _vp, _vp, _vp, _vp,                        # win_ret, win_len, win_code, mean_ret, mean_len, success
                         _vp], ctypes.c_int),                                 # stream
}

lib = _loader.load("libaqua_segments.so", LIB_PATH, "aquaseg", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaseg", AquaSegmentsError)


def last_error():
    return lib.aquaseg_last_error().decode("utf-8", "replace")
