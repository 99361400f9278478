"""ctypes binding of libaqua_lbank.so (include/aqua_lbank.h).  No fallback: if the HIP library is missing or does not
load, importing this module raises -- the learner bank has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_LBANK_LIB", "libaqua_lbank.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
PARAMS = 4739                     # _learner_capi.PARAMS
MAX_BATCH = 1 << 20
MAX_NETWORKS = 4096
MAX_CAPACITY = 2 ** 31 - 1
HYPER_FIELDS = ("gamma", "tau", "lr", "beta1", "beta2", "eps")
HYPER_WORDS = 8                   # doubles per row of the device table
STREAM = 6                        # Philox stream of the minibatch draws
ATTEMPTS = 4

# every symbol include/aqua_lbank.h declares (tests/test_lbank_cpu.py checks the library exports them all)
SYMBOLS = ("aqualbank_version", "aqualbank_last_error", "aqualbank_workspace_bytes", "aqualbank_pack_hyper",
           "aqualbank_update_f32", "aqualbank_draw")


class AquaLearnerBankError(RuntimeError):
    pass


_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_SIGNATURES = {
    "aqualbank_workspace_bytes": ([_i64, _i64], _sz),
    "aqualbank_pack_hyper": ([_vp, _i64, _vp], _ci),
    "aqualbank_update_f32": ([_vp, _vp, _vp, _vp, _vp, _i64,                   # theta, theta_target, m, v, t, P
                              _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,        # s, a, r, s2, d, ok, ld, size
                              _vp, _i64, _ci, _vp,                             # idx, B, strategy, hyper
                              _vp, _vp, _vp, _i64,                             # blob_online, blob_target, perm, blob_floats
                              _vp, _sz,                                        # workspace, workspace_bytes
                              _vp, _vp, _vp, _vp], _ci),                       # idx_out, grad_out, loss, stream
    "aqualbank_draw": ([_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp], _ci),
}

lib = _loader.load("libaqua_lbank.so", LIB_PATH, "aqualbank", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aqualbank", AquaLearnerBankError)


def last_error():
    return lib.aqualbank_last_error().decode("utf-8", "replace")


def pack_hyper(rows):
    """rows: float64 [P][6] (gamma, tau, lr, beta1, beta2, eps per network) -> the table float64 [P][HYPER_WORDS] for the
    device; a row that aqualrn_update_f32 would reject is a ValueError that names the network"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != len(HYPER_FIELDS):
        raise ValueError("expected [P][%d] hyper-parameters, got %s" % (len(HYPER_FIELDS), rows.shape))
    out = np.zeros((rows.shape[0], HYPER_WORDS), dtype=np.float64)
    check(lib.aqualbank_pack_hyper(rows.ctypes.data, rows.shape[0], out.ctypes.data), "aqualbank_pack_hyper")
    return out
