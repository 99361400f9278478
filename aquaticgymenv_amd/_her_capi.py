"""ctypes binding of libaqua_her.so (csrc/aqua_her.h).  No fallback: if the HIP library is missing or does not load,
importing this module raises -- hindsight relabelling of the experience ring has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_HER_LIB", "libaqua_her.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_HORIZON = 64                  # H at most
CHUNK = 8                         # steps whose loads are in flight together
STREAM = 8                        # Philox stream of the relabelling draws
MAX_CAPACITY = (1 << 31) - 1
MAX_NETWORKS = 4096
MAX_BATCH = 1 << 20
MAX_BLOCKS = 2048
BLOCK = 256
NO_SEED = 0                       # the scalar seed of a call that passes the bank's keys
TERM_SUCCESS = 3                  # the termination code of a relabelled success
ACT_U8, ACT_F32X2 = 0, 1

# every symbol csrc/aqua_her.h declares (tests/test_her_cpu.py checks the library exports them all)
SYMBOLS = ("aquaher_version", "aquaher_last_error", "aquaher_threshold", "aquaher_reward", "aquaher_relabel")


class AquaHerError(RuntimeError):
    pass


_vp, _i64, _u64, _int, _dbl, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_float
_SIGNATURES = {
    "aquaher_threshold": ([_dbl, _vp], _int),                                          # ratio, thr
    "aquaher_reward": ([_vp, _vp, _flt, _flt, _vp, _vp], _int),                        # s, s2, gx, gy, r, d
    "aquaher_relabel": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _i64,    # header, s, a, r, s2, d, ok, ring_ld, capacity, kind, N
                         _vp, _i64, _i64, _int, _dbl, _vp, _u64, _vp,                  # idx, P, B, H, ratio, t_dev, seed, seed_dev
                         _vp, _vp, _vp, _vp, _vp, _vp, _i64,                           # out_s, out_a, out_r, out_s2, out_d, out_ok, out_ld
                         _vp, _vp, _vp], _int),                                        # out_k, out_m, stream
}

lib = _loader.load("libaqua_her.so", LIB_PATH, "aquaher", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaher", AquaHerError)


def last_error():
    return lib.aquaher_last_error().decode("utf-8", "replace")


def threshold(ratio):
    """aquaher_threshold(): floor(ratio 2^32), what a draw's first word is compared with (a host computation)"""
    out = _u64(0)
    if lib.aquaher_threshold(float(ratio), ctypes.byref(out)) != 0:
        raise ValueError("aquaher_threshold: %s" % last_error())
    return int(out.value)


def reward(s, s2, gx, gy):
    """aquaher_reward(): (reward, code) of the transition s -> s2 (five float32 each) replayed under the goal (gx, gy), by the
    kernel's own code on the host"""
    a, b = (ctypes.c_float * 5)(*[float(v) for v in s]), (ctypes.c_float * 5)(*[float(v) for v in s2])
    r, d = _flt(0.0), ctypes.c_uint8(0)
    check(lib.aquaher_reward(ctypes.addressof(a), ctypes.addressof(b), float(gx), float(gy), ctypes.byref(r), ctypes.byref(d)), "aquaher_reward")
    return r.value, int(d.value)
