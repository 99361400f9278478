"""ctypes binding of libaqua_episodes.so (include/aqua_episodes.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- episode accounting has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_EPISODES_LIB", "libaqua_episodes.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_WORLDS = 1 << 30
MAX_BLOCKS = 1024
COUNTS = 8                        # uint64 slots of counts[]: logged, by code 1..3, world-steps, three unused
STREAM = 5                        # Philox stream of the exploration draws: the policy's

# every symbol include/aqua_episodes.h declares (tests/test_episodes_cpu.py checks the library exports them all)
SYMBOLS = ("aquaep_version", "aquaep_last_error", "aquaep_workspace_bytes", "aquaep_after_step_f32", "aquaep_explore_u8")


class AquaEpisodesError(RuntimeError):
    pass


_vp, _i64, _u64, _cd, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double, ctypes.c_size_t
_SIGNATURES = {
    "aquaep_workspace_bytes": ([_i64], _sz),
    "aquaep_after_step_f32": ([_vp, _vp, _vp, _i64, _i64,                   # reward, term, time, env_offset, N
                               _vp, _vp, _vp,                               # ret, len, finished
                               _vp, _vp, _vp, _vp, _i64,                    # log_ret, log_len, log_code, log_world, C
                               _vp, _vp, _vp, _cd, _cd,                     # counts, eps_state, eps_out, decay, eps_final
                               _vp, _sz, _vp], ctypes.c_int),               # workspace, workspace_bytes, stream
    "aquaep_explore_u8": ([_vp, _i64, _i64, _vp, _u64, _u64, _vp, _vp],     # action, N, env_offset, eps, seed, tick, tick_base, stream
                          ctypes.c_int),
}

lib = _loader.load("libaqua_episodes.so", LIB_PATH, "aquaep", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaep", AquaEpisodesError)
