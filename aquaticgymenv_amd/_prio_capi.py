"""ctypes binding of libaqua_prio.so (csrc/aqua_prio.h).  No fallback: if the HIP library is missing or does not load,
importing this module raises -- prioritised replay has no CPU path.  The four host functions (pow_, quantise, beta, weight)
compute the device's bits without a device."""
import ctypes

import numpy as np

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_PRIO_LIB", "libaqua_prio.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
FANOUT = 64                       # children per node
FRAC_BITS = 20                    # fraction bits of a leaf
ONE = 1 << FRAC_BITS              # the quantised pi = 1: what pmax starts from
QMAX = (1 << 31) - 1              # the largest leaf
MAX_LEVELS = 7                    # levels at most, the leaves included
LAYOUT_WORDS = 3 + 3 * MAX_LEVELS
STREAM = 7                        # the Philox stream of the descent's draws
MAX_CAPACITY = (1 << 31) - 1
MAX_NETWORKS = 4096
MAX_BATCH = 1 << 20
MAX_BLOCKS = 2048
BLOCK = 256
WAVES = BLOCK // 64               # samples a block of the descent takes per pass

# every symbol csrc/aqua_prio.h declares (tests/test_prio_cpu.py checks the library exports them all)
SYMBOLS = ("aquaprio_version", "aquaprio_last_error", "aquaprio_layout", "aquaprio_pow", "aquaprio_quantise", "aquaprio_beta",
           "aquaprio_weight", "aquaprio_insert", "aquaprio_set", "aquaprio_draw", "aquaprio_update_f32")


class AquaPriorityError(RuntimeError):
    pass


_vp, _i64, _u64, _u32, _int, _dbl, _sz = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_size_t)
_TREE = [_vp, _sz]                                                                      # tree, tree_bytes
_SHAPE = [_i64, _i64, _i64, _i64]                                                       # capacity, N, seg, P
_SIGNATURES = {
    "aquaprio_layout": (_SHAPE + [_vp], _int),
    "aquaprio_pow": ([_dbl, _dbl], _dbl),
    "aquaprio_quantise": ([_dbl, _dbl, _dbl], _u32),
    "aquaprio_beta": ([_u64, _dbl, _i64], _dbl),
    "aquaprio_weight": ([_u64, _u32, _u64, _dbl], _dbl),
    "aquaprio_insert": (_TREE + [_vp] + _SHAPE + [_vp, _vp, _vp], _int),                # pmax | header, ok, stream
    "aquaprio_set": (_TREE + [_vp] + _SHAPE + [_vp, _vp, _i64, _dbl, _dbl, _vp], _int),  # pmax | idx, td, B, alpha, eps, stream
    "aquaprio_draw": (_TREE + _SHAPE + [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _dbl, _i64, _vp], _int),
    # header, t, seed, idx, weight, q_out, B, beta0, anneal, stream
    "aquaprio_update_f32": ([_vp, _vp, _vp, _vp, _vp, _i64,                             # theta, target, m, v, t, P
                             _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,                  # s, a, r, s2, d, ok, ld, size
                             _vp, _i64, _int, _vp,                                      # idx, B, strategy, hyper
                             _vp, _vp, _vp, _i64,                                       # blob_online, blob_target, perm, blob_floats
                             _vp, _sz,                                                  # workspace, workspace_bytes
                             _vp, _vp, _vp, _vp, _vp, _vp], _int),                      # idx_out, grad_out, loss, weight, td_out, stream
}

lib = _loader.load("libaqua_prio.so", LIB_PATH, "aquaprio", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaprio", AquaPriorityError)


def last_error():
    return lib.aquaprio_last_error().decode("utf-8", "replace")


def layout(capacity, N, seg, P):
    """aquaprio_layout() -> {"levels", "bytes", "leaves", "n": [...], "stride": [...], "offset": [...]} (a host computation)"""
    out = np.zeros(LAYOUT_WORDS, dtype=np.int64)
    check(lib.aquaprio_layout(int(capacity), int(N), int(seg), int(P), out.ctypes.data), "aquaprio_layout")
    levels = int(out[0])
    rows = out[3:3 + 3 * levels].reshape(levels, 3)
    return {"levels": levels, "bytes": int(out[1]), "leaves": int(out[2]), "n": [int(x) for x in rows[:, 0]],
            "stride": [int(x) for x in rows[:, 1]], "offset": [int(x) for x in rows[:, 2]]}


def pow_(x, e):
    """aquaprio_pow(): the library's x^e (a host computation)"""
    out = lib.aquaprio_pow(float(x), float(e))
    if out < 0.0:
        raise ValueError("aquaprio_pow: %s" % last_error())
    return out


def quantise(td, alpha, eps):
    """aquaprio_quantise(): the leaf of a TD error (a host computation)"""
    out = int(lib.aquaprio_quantise(float(td), float(alpha), float(eps)))
    if out == 0:
        raise ValueError("aquaprio_quantise: %s" % last_error())
    return out


def beta(t, beta0, anneal):
    """aquaprio_beta(): the importance exponent after t updates (a host computation)"""
    out = lib.aquaprio_beta(int(t), float(beta0), int(anneal))
    if out < 0.0:
        raise ValueError("aquaprio_beta: %s" % last_error())
    return out


def weight(size, q, T, beta_):
    """aquaprio_weight(): the raw importance weight (size q / T)^-beta (a host computation)"""
    out = lib.aquaprio_weight(int(size), int(q), int(T), float(beta_))
    if out < 0.0:
        raise ValueError("aquaprio_weight: %s" % last_error())
    return out
