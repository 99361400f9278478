"""ctypes binding of libaqua_render.so (include/aqua_render.h).  No fallback: if the HIP library is missing or does not
load, importing this module raises -- frames have no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_RENDER_LIB", "libaqua_render.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
MAX_WORLDS = 1 << 30
MAX_BLOCKS = (1 << 24) - 1        # blocks of one frames launch: M x tiles(M, S) at most
MAX_ROWS = 64                     # obstacle rows per table
MIN_SIZE, MAX_SIZE = 16, 1000     # frame side S, a multiple of 4
OVERLAY_ROWS = 4                  # tl, tr, icc_x, icc_y

# every symbol include/aqua_render.h declares (tests/test_render_cpu.py checks the library exports them all)
SYMBOLS = ("aquarnd_version", "aquarnd_last_error", "aquarnd_overlay_u8", "aquarnd_overlay_f32x2", "aquarnd_frames_u8")


class AquaRenderError(RuntimeError):
    pass


_vp, _i64, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_SIGNATURES = {
    "aquarnd_overlay_u8": ([_vp, _i64, _i64, _vp, _vp, _i64, _vp], _int),            # state, ld, N, action, overlay, overlay_ld, stream
    "aquarnd_overlay_f32x2": ([_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp], _int),   # state, ld, N, action, action_ld, overlay, overlay_ld, stream
    "aquarnd_frames_u8": ([_vp, _i64, _i64, _vp, _i64,                               # state, ld, N, overlay, overlay_ld
                           _vp, _int, _int, _int,                                    # rows, K, per_world, waves
                           _vp, _i64, _int, _vp, _sz, _vp], _int),                   # worlds, M, S, out, out_bytes, stream
}

lib = _loader.load("libaqua_render.so", LIB_PATH, "aquarnd", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquarnd", AquaRenderError)
