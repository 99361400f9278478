"""ctypes binding of libaqua_policy.so (include/aqua_policy.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- the Q-network has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_POLICY_LIB", "libaqua_policy.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
SHAPES = (5, 64, 64, 3)           # main/impl/dqn.py:301-314
STREAM = 5                        # Philox stream of the epsilon-greedy draws

# every symbol include/aqua_policy.h declares (tests/test_qpolicy_cpu.py checks the library exports them all)
SYMBOLS = ("aquapol_version", "aquapol_last_error", "aquapol_weights_bytes", "aquapol_pack_weights", "aquapol_act_f32")


class AquaPolicyError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cf, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_SIGNATURES = {
    "aquapol_weights_bytes": (None, _sz),
    "aquapol_pack_weights": ([_vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_ci), _vp, _sz], _ci),
    "aquapol_act_f32": ([_vp, _vp, _i64, _ci, _i64, _i64, _cf, _u64, _u64, _vp, _vp, _vp, _i64, _vp, _vp], _ci),
}

lib = _loader.load("libaqua_policy.so", LIB_PATH, "aquapol", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquapol", AquaPolicyError)


def pack_weights(layers):
    """layers: [(kernel [in, out], bias [out])] * 3 as tf_import.dense_stack() returns them -> numpy uint8 array holding
    the device-format blob.  Another architecture than 5-64-64-3: ValueError."""
    import numpy as np
    layers = list(layers)
    if len(layers) != 3:
        raise ValueError("the Q-network has three dense layers, got %d" % len(layers))
    ks = [np.ascontiguousarray(k, dtype=np.float32) for k, _ in layers]
    bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for _, b in layers]
    for k, b in zip(ks, bs):
        if k.ndim != 2 or b.shape[0] != k.shape[1]:
            raise ValueError("kernel %s / bias %s: expected [in, out] and [out]" % (k.shape, b.shape))
    if ks[1].shape[0] != ks[0].shape[1] or ks[2].shape[0] != ks[1].shape[1]:
        raise ValueError("layer widths do not chain: %s" % ([k.shape for k in ks],))
    shapes = (ctypes.c_int * 4)(ks[0].shape[0], ks[0].shape[1], ks[1].shape[1], ks[2].shape[1])
    n = lib.aquapol_weights_bytes()
    blob = np.zeros(n, dtype=np.uint8)
    check(lib.aquapol_pack_weights(ks[0].ctypes.data, bs[0].ctypes.data, ks[1].ctypes.data, bs[1].ctypes.data,
                                   ks[2].ctypes.data, bs[2].ctypes.data, shapes, blob.ctypes.data, n), "aquapol_pack_weights")
    return blob
