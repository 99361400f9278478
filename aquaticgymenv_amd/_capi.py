"""ctypes binding of libaqua_hip.so (include/aqua_hip.h).  No fallback: if the HIP library is
missing or does not load, importing this module raises -- the product has no CPU path."""
import ctypes

from . import _loader

# AQUA_HIP_LIB selects a tuning build of the same library (aquaticgymenv_amd/build.py --variants)
LIB_PATH = _loader.lib_path("AQUA_HIP_LIB", "libaqua_hip.so")

ABI_VERSION = 8
ACT_U8, ACT_I32, ACT_I64, ACT_F32X2, ACT_SAMPLE_D, ACT_SAMPLE_C, ACT_BEARING = range(7)
TERM_NONE, TERM_COLLIDED, TERM_TIME, TERM_SUCCESS = range(4)
MAX_OBSTACLES = 64

# every symbol include/aqua_hip.h declares (tests/test_capi_cpu.py checks the library exports them all)
SYMBOLS = (
    "aqua_version", "aqua_last_error", "aqua_obstacle_blob_bytes", "aqua_pack_obstacles", "aqua_step_f32",
    "aqua_reset_f32", "aqua_rollout_f32", "aqua_rollout_fused_f32", "aqua_tick_advance", "aqua_graph_begin",
    "aqua_graph_end", "aqua_graph_launch", "aqua_graph_upload", "aqua_graph_destroy",
    "aqua_discrete_constants", "aqua_obs_norm_f32",
    "aqua_ring_write_f32", "aqua_ring_write_u8", "aqua_pack_tables", "aqua_tables32_floats", "aqua_step_tables_f32", "aqua_reset_tables_f32",
    "aqua_event_create", "aqua_event_record", "aqua_event_elapsed_ms", "aqua_event_destroy", "aqua_graph_end_timed", "aqua_rollout_tables_f32",
    "aqua_rollout_tables_fused_f32",
    "aqua_ipc_buffer_create", "aqua_ipc_buffer_ptr", "aqua_ipc_buffer_handle", "aqua_ipc_buffer_destroy", "aqua_ipc_open",
    "aqua_ipc_close", "aqua_copy_async", "aqua_copy_fanout_async", "aqua_rollout_events_f32",
)
IPC_HANDLE_BYTES = 64
COPY_ENGINE_WAVES, COPY_ENGINE_DMA = 0, 1


class AquaParams(ctypes.Structure):
    _fields_ = [("waves", ctypes.c_int32), ("continuous", ctypes.c_int32), ("random_boat", ctypes.c_int32),
                ("random_goal", ctypes.c_int32), ("time_limit", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class AquaError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cf, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_pp, _pvp = ctypes.POINTER(AquaParams), ctypes.POINTER(ctypes.c_void_p)
# symbol: (argtypes, restype) as include/aqua_hip.h declares them
_SIGNATURES = {
    "aqua_obstacle_blob_bytes": ([_ci], _sz),
    "aqua_pack_obstacles": ([_vp, _ci, _vp, _sz], _ci),
    "aqua_step_f32": ([_pp, _vp, _ci, _i64, _i64, _vp, _i64, _vp, _vp, _ci, _i64, _vp, _i64, _u64, _u64, _vp, _vp, _vp, _vp,
                       _vp, _ci, _vp], _ci),
    "aqua_reset_f32": ([_pp, _vp, _ci, _i64, _i64, _vp, _i64, _vp, _vp, _u64, _u64, _vp, _vp], _ci),
    "aqua_rollout_f32": ([_pp, _vp, _ci, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _ci, _i64, _i64, _u64, _u64, _vp, _vp, _vp,
                          _i64, _vp, _i64, _vp, _ci, _ci, _vp], _ci),
    "aqua_rollout_events_f32": ([_pp, _vp, _ci, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _ci, _i64, _i64, _u64, _u64, _vp, _vp, _vp,
                                 _i64, _vp, _i64, _vp, _ci, _ci, _vp, _vp, _vp], _ci),
    "aqua_rollout_fused_f32": ([_pp, _vp, _ci, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _ci, _i64, _i64, _u64, _u64, _vp,
                                _vp, _vp, _i64, _ci, _vp], _ci),
    "aqua_tick_advance": ([_vp, _u64, _vp], _ci),
    "aqua_obs_norm_f32": ([_vp, _i64, _i64, _vp, _vp, _vp], _ci),
    "aqua_ring_write_f32": ([_vp, _i64, _i64, _i64, _vp, _i64, _ci, _i64, _vp], _ci),
    "aqua_ring_write_u8": ([_vp, _i64, _i64, _i64, _vp, _i64, _ci, _i64, _vp], _ci),
    "aqua_pack_tables": ([_vp, _ci, _i64, _i64, _vp, _vp, ctypes.POINTER(_cf)], _ci),
    "aqua_tables32_floats": ([_ci, _i64], _sz),
    "aqua_step_tables_f32": ([_pp, _vp, _vp, _ci, _i64, _cf, _i64, _i64, _vp, _i64, _vp, _vp, _ci, _i64, _vp, _i64,
                              _u64, _u64, _vp, _vp, _vp, _vp, _vp, _ci, _vp], _ci),
    "aqua_rollout_tables_f32": ([_pp, _vp, _vp, _ci, _i64, _cf, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _ci, _i64, _i64,
                                 _u64, _u64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _ci, _ci, _vp], _ci),
    "aqua_rollout_tables_fused_f32": ([_pp, _vp, _vp, _ci, _i64, _cf, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _ci, _i64, _i64,
                                       _u64, _u64, _vp, _vp, _vp, _i64, _ci, _vp], _ci),
    "aqua_reset_tables_f32": ([_pp, _vp, _ci, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _u64, _u64, _vp, _vp], _ci),
    "aqua_graph_begin": ([_vp], _ci),
    "aqua_graph_end": ([_vp, _pvp], _ci),
    "aqua_graph_launch": ([_vp, _vp], _ci),
    "aqua_graph_upload": ([_vp, _vp], _ci),
    "aqua_graph_destroy": ([_vp], _ci),
    "aqua_event_create": ([_pvp], _ci),
    "aqua_event_record": ([_vp, _vp], _ci),
    "aqua_event_elapsed_ms": ([_vp, _vp, ctypes.POINTER(_cf)], _ci),
    "aqua_event_destroy": ([_vp], _ci),
    "aqua_graph_end_timed": ([_vp, _pvp, _vp, _vp], _ci),
    "aqua_ipc_buffer_create": ([_sz, _pvp], _ci),
    "aqua_ipc_buffer_ptr": ([_vp], _vp),
    "aqua_ipc_buffer_handle": ([_vp, ctypes.c_char_p], _ci),
    "aqua_ipc_buffer_destroy": ([_vp], _ci),
    "aqua_ipc_open": ([ctypes.c_char_p, _pvp], _ci),
    "aqua_ipc_close": ([_vp], _ci),
    "aqua_copy_async": ([_vp, _vp, _sz, _ci, _vp], _ci),
    "aqua_copy_fanout_async": ([_pvp, _ci, _vp, _sz, _vp], _ci),
    "aqua_discrete_constants": ([ctypes.POINTER(_cf)], None),
}


def _load():
    """the library at LIB_PATH as it is now (tools/overlap_roles.py loads the tuning builds beside the shipped one)"""
    return _loader.load("libaqua_hip.so", LIB_PATH, "aqua", ABI_VERSION, _SIGNATURES)


lib = _load()
check = _loader.checker(lib, "aqua", AquaError)


def pack_obstacles(rows):
    """rows: numpy float64 [K][5] -> bytes of the device-format blob (empty for K == 0)."""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 5)
    k = rows.shape[0]
    if k > MAX_OBSTACLES:
        raise ValueError("at most %d obstacles, got %d" % (MAX_OBSTACLES, k))
    n = lib.aqua_obstacle_blob_bytes(k)
    buf = (ctypes.c_uint8 * max(n, 1))()
    check(lib.aqua_pack_obstacles(rows.ctypes.data, k, ctypes.addressof(buf), n), "aqua_pack_obstacles")
    return bytes(buf)[:n]


def discrete_constants():
    out = (ctypes.c_float * 9)()
    lib.aqua_discrete_constants(out)
    return [float(v) for v in out]
