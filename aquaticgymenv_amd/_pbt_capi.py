"""ctypes binding of libaqua_pbt.so (aquaticgymenv_amd/include/aqua_pbt.h).  No fallback: if the HIP library is missing or
does not load, importing this module raises -- selection among the networks of a population has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_PBT_LIB", "libaqua_pbt.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_NETWORKS = 4096
PARAMS = 4739                     # _lbank_capi.PARAMS
MAX_BLOB = 1 << 20
HEADER = 4                        # uint64 slots of header[]: calls, replaced, replaced by the last call, scored by the last call
COUNTS = 8                        # _segments_capi.COUNTS
HYPER_WORDS = 8                   # _lbank_capi.HYPER_WORDS
HYPER_GAMMA, HYPER_LR = 0, 2      # the words of a row of the learner bank's table that selection perturbs
STREAM = 7                        # Philox stream of the selection draws

# every symbol the header declares (tests/test_pbt_cpu.py checks the library exports them all)
SYMBOLS = ("aquapbt_version", "aquapbt_last_error", "aquapbt_select")


class AquaSelectionError(RuntimeError):
    pass


_vp, _i64, _u64, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
_SIGNATURES = {
    "aquapbt_select": ([_vp, _vp, _i64,                                      # score, seg_counts, P
                        _vp, _vp, _vp, _vp,                                  # header, mark, origin, parent
                        _vp, _vp, _vp, _vp, _vp,                             # theta, theta_target, m, v, t
                        _vp, _vp, _i64,                                      # blob_online, blob_target, blob_floats
                        _vp, _vp, _vp,                                       # hyper, eps_state, eps_out
                        _f64, _i64, _i64, _u64,                              # fraction, ready, every, seed
                        _f64, _f64, _f64, _f64,                              # lr_factor0, lr_factor1, lr_lo, lr_hi
                        _f64, _f64, _f64, _f64,                              # gamma_factor0, gamma_factor1, gamma_lo, gamma_hi
                        _vp], ctypes.c_int),                                 # stream
}

lib = _loader.load("libaqua_pbt.so", LIB_PATH, "aquapbt", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquapbt", AquaSelectionError)


def last_error():
    return lib.aquapbt_last_error().decode("utf-8", "replace")
