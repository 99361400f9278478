"""ctypes binding of libaqua_episodes.so (include/aqua_episodes.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- episode accounting has no CPU path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AQUA_EPISODES_LIB") or os.path.join(_HERE, "lib", "libaqua_episodes.so")

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


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libaqua_episodes.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`python -m aquaticgymenv_amd.build` (needs hipcc); there is no CPU fallback")
    # torch's libamdhip64 first, so that this library's NEEDED entry resolves to the same runtime (see _capi.py)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64, u64, ci, cd = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
    lib.aquaep_version.restype = ci
    lib.aquaep_last_error.restype = ctypes.c_char_p
    lib.aquaep_workspace_bytes.argtypes = [i64]
    lib.aquaep_workspace_bytes.restype = ctypes.c_size_t
    lib.aquaep_after_step_f32.argtypes = [vp, vp, vp, i64, i64,               # reward, term, time, env_offset, N
                                          vp, vp, vp,                         # ret, len, finished
                                          vp, vp, vp, vp, i64,                # log_ret, log_len, log_code, log_world, C
                                          vp, vp, vp, cd, cd,                 # counts, eps_state, eps_out, decay, eps_final
                                          vp, ctypes.c_size_t, vp]            # workspace, workspace_bytes, stream
    lib.aquaep_after_step_f32.restype = ci
    lib.aquaep_explore_u8.argtypes = [vp, i64, i64, vp, u64, u64, vp, vp]     # action, N, env_offset, eps, seed, tick, tick_base, stream
    lib.aquaep_explore_u8.restype = ci
    if lib.aquaep_version() != ABI_VERSION:
        raise ImportError("libaqua_episodes.so ABI %d != binding %d: rebuild" % (lib.aquaep_version(), ABI_VERSION))
    return lib


lib = _load()


def check(rc, what):
    if rc != 0:
        msg = lib.aquaep_last_error().decode("utf-8", "replace")
        if rc == E_INVALID:
            raise ValueError("%s: %s" % (what, msg))
        raise AquaEpisodesError("%s failed (code %d): %s" % (what, rc, msg))
