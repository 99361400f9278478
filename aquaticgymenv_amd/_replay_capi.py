"""ctypes binding of libaqua_replay.so (include/aqua_replay.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- the device-cursor experience ring has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_REPLAY_LIB", "libaqua_replay.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
HEADER_WORDS = 4                  # int64: cursor, size, first slot of the batch opened last, batches closed
MAX_CAPACITY = (1 << 31) - 1
MAX_BATCH = 1 << 20
MAX_BLOCKS = 2048
BLOCK = 256
ATTEMPTS = 4
STREAM = 6                        # Philox stream of the minibatch draws: the learner's
ACT_U8, ACT_F32X2 = 0, 1

# every symbol include/aqua_replay.h declares (tests/test_replay_cpu.py checks the library exports them all)
SYMBOLS = ("aquarpl_version", "aquarpl_last_error", "aquarpl_open", "aquarpl_close", "aquarpl_draw", "aquarpl_gather")


class AquaReplayError(RuntimeError):
    pass


_vp, _i64, _u64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int
_SIGNATURES = {
    "aquarpl_open": ([_vp, _vp, _vp, _vp, _i64, _i64,                        # header, s, a, ok, ring_ld, capacity
                      _vp, _i64, _vp, _int, _i64,                            # obs, obs_ld, action, action_kind, action_ld
                      _vp, _i64, _vp], _int),                                # time, N, stream
    "aquarpl_close": ([_vp, _vp, _vp, _vp, _i64, _i64,                       # header, r, s2, d, ring_ld, capacity
                       _vp, _vp, _i64, _vp, _i64, _vp], _int),               # reward, obs, obs_ld, term, N, stream
    "aquarpl_draw": ([_vp, _vp, _i64, _vp, _u64, _vp, _i64, _vp], _int),     # header, ok, capacity, t_dev, seed, idx, B, stream
    "aquarpl_gather": ([_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int,   # idx, B, s, a, r, s2, d, ok, ring_ld, capacity, kind
                        _vp, _vp, _vp, _vp, _vp, _vp, _vp], _int),           # out_s, out_a, out_r, out_s2, out_done, out_valid, stream
}

lib = _loader.load("libaqua_replay.so", LIB_PATH, "aquarpl", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquarpl", AquaReplayError)
