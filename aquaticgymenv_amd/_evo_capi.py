"""ctypes binding of libaqua_evo.so (csrc/aqua_evo.h).  No fallback: if the HIP library is missing or does not load,
importing this module raises -- evolution strategies on a bank have no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_EVO_LIB", "libaqua_evo.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
PARAMS = 4739                     # _learner_capi.PARAMS
MAX_NETWORKS = 4096
STREAM = 9                        # Philox stream of the noise
FIX_BITS = 20
CLAMP = 2048
NOISE_OFFSET = 524280
C = float.fromhex("0x1.3988e1412ed76p-17")
MAX_BLOB = 1 << 20
MAX_WORLDS = (1 << 31) - 1
BLOCK = 256
MAX_BLOCKS = 1024                 # of the accumulation: grid-stride above BLOCK * MAX_BLOCKS items
MEAN_RETURN, SUCCESS_RATE = 0, 1
KINDS = {"mean_return": MEAN_RETURN, "success_rate": SUCCESS_RATE}
ADAM, SGD = 0, 1
OPTIMIZERS = {"adam": ADAM, "sgd": SGD}
HEADER = 8                        # uint64 words of header[]: generation, tells, stepped, best, ranked, three unused
H_GENERATION, H_TELLS, H_STEPPED, H_BEST, H_RANKED = range(5)
NO_SLOT = (1 << 64) - 1
ACC = 3                           # int64 words of the workspace per segment: sum, count, successes

# every symbol csrc/aqua_evo.h declares (tests/test_evo_cpu.py checks the library exports them all)
SYMBOLS = ("aquaevo_version", "aquaevo_last_error", "aquaevo_noise", "aquaevo_quantise", "aquaevo_key", "aquaevo_step_param",
           "aquaevo_ask", "aquaevo_fitness", "aquaevo_tell")


class AquaEvoError(RuntimeError):
    pass


_vp, _i64, _u64, _int, _dbl, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_float
_u32 = ctypes.c_uint32
_SIGNATURES = {
    "aquaevo_noise": ([_u64, _u64, _u32, _u32], ctypes.c_int32),                      # seed, g, j, i
    "aquaevo_quantise": ([_flt], _i64),
    "aquaevo_key": ([_flt], _u32),
    "aquaevo_step_param": ([_i64, _i64, _dbl, _dbl, _dbl, _dbl, _dbl, _dbl, _int, _u64, _vp, _vp], _int),
    "aquaevo_ask": ([_vp, _vp, _vp, _i64, _dbl, _u64, _vp, _i64, _vp], _int),          # theta, perm, header, P, sigma, seed, blob, blob_floats, stream
    "aquaevo_fitness": ([_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int,   # log_ret, log_code, log_world, C, counts, ret, finished,
                         _vp, _vp, _vp, _vp], _int),                                        # env_offset, N, seg, P, kind, acc, fitness, episodes, stream
    "aquaevo_tell": ([_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _u64, _dbl, _dbl, _dbl, _dbl, _dbl, _int,   # fitness, P, header, theta, m, v, t, sigma,
                      _vp, _vp, _vp, _vp], _int),                                   # seed, lr, beta1, beta2, eps, weight_decay, optimizer, rank2, weights, grad_out, stream
}

lib = _loader.load("libaqua_evo.so", LIB_PATH, "aquaevo", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aquaevo", AquaEvoError)


def last_error():
    return lib.aquaevo_last_error().decode("utf-8", "replace")


def noise(seed, g, j, i):
    """aquaevo_noise(): the integer numerator n of the noise of (generation g, pair j, parameter i); eps = n * C"""
    return int(lib.aquaevo_noise(int(seed) & NO_SLOT, int(g) & NO_SLOT, int(j), int(i)))


def quantise(ret):
    """aquaevo_quantise(): a return in 2^-20 fixed point, by the kernel's own code on the host"""
    return int(lib.aquaevo_quantise(_flt(ret)))


def key(fitness):
    """aquaevo_key(): the ranking key of a float32 fitness, by its bits"""
    return int(lib.aquaevo_key(_flt(fitness)))


def key_of_bits(u):
    """aquaevo_key() of the float32 with the bit pattern u (a NaN's payload survives: the float is passed by its bits)"""
    x = _flt.from_buffer_copy(_u32(int(u) & 0xFFFFFFFF))
    return int(lib.aquaevo_key(x))


def step_param(G, H, sigma, lr, beta1, beta2, eps, weight_decay, optimizer, t, theta, m, v):
    """aquaevo_step_param(): one parameter's optimiser step by the kernel's own code on the host
    -> (theta', m', v', grad) with the first three float32 values as Python floats"""
    io = (ctypes.c_float * 3)(theta, m, v)
    grad = _dbl(0.0)
    check(lib.aquaevo_step_param(int(G), int(H), float(sigma), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                 int(optimizer), int(t), ctypes.addressof(io), ctypes.addressof(grad)), "aquaevo_step_param")
    return io[0], io[1], io[2], grad.value
