"""ctypes binding of libaqua_fastpol.so (csrc/aqua_fastpol.h).  No fallback: if the HIP library is missing or does not
load, importing this module raises -- the fast acting path has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_FASTPOL_LIB", "libaqua_fastpol.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
SHAPES = (5, 64, 64, 3)           # main/impl/dqn.py:301-314
STREAM = 5                        # Philox stream of the epsilon-greedy draws
MAX_NETWORKS = 65536
PART_HI, PART_LO, PART_BITS0, PART_BITS1 = 0, 1, 2, 3

# every symbol csrc/aqua_fastpol.h declares (tests/test_fastpol_cpu.py checks the library exports them all)
SYMBOLS = ("aquafast_version", "aquafast_last_error", "aquafast_weights_bytes", "aquafast_map", "aquafast_pack_host",
           "aquafast_refresh", "aquafast_act_f16")


class AquaFastError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cf, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_SIGNATURES = {
    "aquafast_weights_bytes": (None, _sz),
    "aquafast_map": ([_vp, _sz], _ci),
    "aquafast_pack_host": ([_vp, _vp, _sz], _ci),
    "aquafast_refresh": ([_vp, _i64, _vp, _vp, _i64, _vp], _ci),
    "aquafast_act_f16": ([_vp, _i64, _i64, _vp, _i64, _ci, _i64, _i64, _cf, _vp, _u64, _u64, _vp, _vp, _vp, _i64, _vp, _vp], _ci),
}

lib = _loader.load("libaqua_fastpol.so", LIB_PATH, "aquafast", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquafast", AquaFastError)


def last_error():
    return lib.aquafast_last_error().decode("utf-8", "replace")


def blob_map():
    """aquafast_map(): int32 [aquafast_weights_bytes() / 2], for every 16-bit element of a fast blob 4 * (float index in
    the float32 acting blob) + PART_*, or -1 for padding"""
    import numpy as np
    m = np.empty(lib.aquafast_weights_bytes() // 2, dtype=np.int32)
    check(lib.aquafast_map(m.ctypes.data, m.nbytes), "aquafast_map")
    return m


def pack_host(blob):
    """blob: the float32 acting blob of one network on the host (numpy uint8 or float32, as _policy_capi.pack_weights()
    returns it) -> its fast blob, numpy uint8 [aquafast_weights_bytes()]"""
    import numpy as np
    from . import _policy_capi
    blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    if blob.nbytes != _policy_capi.lib.aquapol_weights_bytes():
        raise ValueError("a float32 blob has %d bytes, got %d" % (_policy_capi.lib.aquapol_weights_bytes(), blob.nbytes))
    out = np.zeros(lib.aquafast_weights_bytes(), dtype=np.uint8)
    check(lib.aquafast_pack_host(blob.ctypes.data, out.ctypes.data, out.nbytes), "aquafast_pack_host")
    return out
