"""ctypes binding of libaqua_qmap.so (aquaticgymenv_amd/csrc/aqua_qmap.h).  No fallback: if the HIP library is missing or
does not load, importing this module raises -- Q-value maps have no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_QMAP_LIB", "libaqua_qmap.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
ACTIONS = 3
MAX_NETWORKS = 65536              # _bank_capi.MAX_NETWORKS
MAX_GOALS = 65536
MAX_SIDE = 65536                  # W and H
MAX_SECTORS = 4096
MAX_STATES = 1 << 30              # S * H * W
MAX_TOTAL = 1 << 40               # P * G * S * H * W
TILE = 32                         # states of an item

# every symbol the header declares (tests/test_qmaps_cpu.py checks the library exports them all)
SYMBOLS = ("aquaqmap_version", "aquaqmap_last_error", "aquaqmap_weights_bytes", "aquaqmap_items", "aquaqmap_maps_f32")


class AquaMapError(RuntimeError):
    pass


_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_SIGNATURES = {
    "aquaqmap_weights_bytes": (None, _sz),
    "aquaqmap_items": ([_i64, _i64, _i64, _i64, _i64], _i64),                # P, G, H, W, S
    "aquaqmap_maps_f32": ([_vp, _i64,                                        # bank_dev, P
                           _vp, _i64, _vp, _i64, _vp, _i64,                  # xs, W, ys, H, angles, S
                           _vp, _i64,                                        # goals, G
                           _vp, _vp, _vp, _vp], _ci),                        # action, value, q, stream
}

lib = _loader.load("libaqua_qmap.so", LIB_PATH, "aquaqmap", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaqmap", AquaMapError)


def last_error():
    return lib.aquaqmap_last_error().decode("utf-8", "replace")
