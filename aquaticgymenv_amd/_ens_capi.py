"""ctypes binding of libaqua_ens.so (aquaticgymenv_amd/csrc/aqua_ens.h).  No fallback: if the HIP library is missing or
does not load, importing this module raises -- the ensemble policy has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_ENS_LIB", "libaqua_ens.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
STREAM = 5                        # Philox stream of the epsilon-greedy draws: the policy's
ACTIONS = 3
MAX_NETWORKS = 65536              # _bank_capi.MAX_NETWORKS
MEAN, VOTE = 0, 1
MODES = {"mean": MEAN, "vote": VOTE}
GROUP = 4                         # tiles of 32 worlds a wavefront carries through the member loop
TILE = 32

# every symbol the header declares (tests/test_ens_cpu.py checks the library exports them all)
SYMBOLS = ("aquaens_version", "aquaens_last_error", "aquaens_weights_bytes", "aquaens_shape", "aquaens_act_f32")


class AquaEnsError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cf, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_SIGNATURES = {
    "aquaens_weights_bytes": (None, _sz),
    "aquaens_shape": ([_i64, _ci, _vp], _ci),                                # N, cus, out[3]
    "aquaens_act_f32": ([_vp, _i64, _vp, _ci,                                # bank_dev, networks, member_dev, mode
                         _vp, _i64, _ci, _i64, _i64,                         # in, ld, in_is_normalised, N, env_offset
                         _cf, _vp, _u64, _u64, _vp,                          # epsilon, epsilon_dev, seed, tick, tick_base_dev
                         _vp, _vp, _i64, _vp,                                # action, q, q_ld, q_taken
                         _vp, _vp, _i64, _vp], _ci),                         # variance, votes, x_ld, stream
}

lib = _loader.load("libaqua_ens.so", LIB_PATH, "aquaens", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaens", AquaEnsError)


def last_error():
    return lib.aquaens_last_error().decode("utf-8", "replace")


def shape(N, cus):
    """the launch aquaens_act_f32 makes for N worlds on a device of `cus` compute units (no device needed) ->
    (blocks, groups of GROUP tiles, the most groups one wavefront takes)"""
    out = (ctypes.c_int64 * 3)()
    check(lib.aquaens_shape(int(N), int(cus), ctypes.addressof(out)), "aquaens_shape")
    return tuple(int(v) for v in out)
