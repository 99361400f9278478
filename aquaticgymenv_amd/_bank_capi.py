"""ctypes binding of libaqua_bank.so (include/aqua_bank.h).  No fallback: if the HIP library is missing or does not
load, importing this module raises -- the Q-network bank has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_BANK_LIB", "libaqua_bank.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
SHAPES = (5, 64, 64, 3)           # main/impl/dqn.py:301-314
STREAM = 5                        # Philox stream of the epsilon-greedy draws
MAX_NETWORKS = 65536

# every symbol include/aqua_bank.h declares (tests/test_qbank_cpu.py checks the library exports them all)
SYMBOLS = ("aquabank_version", "aquabank_last_error", "aquabank_weights_bytes", "aquabank_items", "aquabank_unpack_weights",
           "aquabank_act_f32")


class AquaBankError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cf, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_SIGNATURES = {
    "aquabank_weights_bytes": (None, _sz),
    "aquabank_items": ([_i64, _i64], _i64),
    "aquabank_unpack_weights": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], _ci),
    "aquabank_act_f32": ([_vp, _i64, _i64, _vp, _i64, _ci, _i64, _i64, _cf, _vp, _u64, _u64, _vp, _vp, _vp, _i64, _vp, _vp], _ci),
}

lib = _loader.load("libaqua_bank.so", LIB_PATH, "aquabank", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquabank", AquaBankError)


def last_error():
    return lib.aquabank_last_error().decode("utf-8", "replace")


def unpack_weights(blob):
    """blob: one slot of the bank on the host (numpy uint8 or float32, aquabank_weights_bytes() bytes) ->
    [(kernel [in, out], bias [out])] * 3 as tf_import.dense_stack() returns them: the inverse of _policy_capi.pack_weights"""
    import numpy as np
    blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    if blob.nbytes != lib.aquabank_weights_bytes():
        raise ValueError("a slot has %d bytes, got %d" % (lib.aquabank_weights_bytes(), blob.nbytes))
    ks = [np.zeros((SHAPES[i], SHAPES[i + 1]), dtype=np.float32) for i in range(3)]
    bs = [np.zeros(SHAPES[i + 1], dtype=np.float32) for i in range(3)]
    check(lib.aquabank_unpack_weights(blob.ctypes.data, ks[0].ctypes.data, bs[0].ctypes.data, ks[1].ctypes.data, bs[1].ctypes.data,
                                      ks[2].ctypes.data, bs[2].ctypes.data), "aquabank_unpack_weights")
    return list(zip(ks, bs))
