"""ctypes binding of libaqua_nstep.so (csrc/aqua_nstep.h).  No fallback: if the HIP library is missing or does not load,
importing this module raises -- the n-step fold of the experience ring has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_NSTEP_LIB", "libaqua_nstep.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_STEPS = 32                    # n at most
CHUNK = 8                         # steps whose loads are in flight together
MAX_CAPACITY = (1 << 31) - 1
MAX_NETWORKS = 4096
MAX_BATCH = 1 << 20
MAX_BLOCKS = 2048
BLOCK = 256
HYPER_WORDS = 8                   # doubles per row of the learner bank's table; word 0 is gamma
NO_GAMMA = -1.0                   # the scalar gamma of a call that passes the table
ACT_U8, ACT_F32X2 = 0, 1

# every symbol csrc/aqua_nstep.h declares (tests/test_nstep_cpu.py checks the library exports them all)
SYMBOLS = ("aquanst_version", "aquanst_last_error", "aquanst_discount", "aquanst_fold")


class AquaNStepError(RuntimeError):
    pass


_vp, _i64, _int, _dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_SIGNATURES = {
    "aquanst_discount": ([_dbl, _int], _dbl),
    "aquanst_fold": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _i64,       # header, s, a, r, s2, d, ok, ring_ld, capacity, kind, N
                      _vp, _i64, _i64, _int, _dbl, _vp,                                # idx, P, B, n, gamma, hyper_dev
                      _vp, _vp, _vp, _vp, _vp, _vp, _i64,                              # out_s, out_a, out_r, out_s2, out_d, out_ok, out_ld
                      _vp, _vp, _vp], _int),                                           # out_len, hyper_out, stream
}

lib = _loader.load("libaqua_nstep.so", LIB_PATH, "aquanst", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquanst", AquaNStepError)


def last_error():
    return lib.aquanst_last_error().decode("utf-8", "replace")


def discount(gamma, n):
    """aquanst_discount(): the bootstrap discount of an n-step target, float32(gamma) to the n-th power by n - 1 rounded
    double products (a host computation)"""
    out = lib.aquanst_discount(float(gamma), int(n))
    if out < 0.0:
        raise ValueError("aquanst_discount: %s" % last_error())
    return out
