"""ctypes binding of libaqua_learner.so (include/aqua_learner.h).  No fallback: if the HIP library is missing or does
not load, importing this module raises -- the DQN update has no CPU path."""
import ctypes

from . import _loader

LIB_PATH = _loader.lib_path("AQUA_LEARNER_LIB", "libaqua_learner.so")

ABI_VERSION = 1
E_INVALID, E_ALIGN, E_NODEVICE = -1, -2, -3
PARAMS = 4739                     # k0 [5][64], b0 [64], k1 [64][64], b1 [64], k2 [64][3], b2 [3]
MAX_BATCH = 1 << 20
STREAM = 6                        # Philox stream of the minibatch draws
STRATEGIES = {"double_ref": 0, "double": 1, "fixed": 2, "standard": 3}
LOSS_REFERENCE = 16               # AQUALRN_LOSS_REFERENCE, OR-ed into the strategy argument
LOSSES = {"mse": 0, "reference": LOSS_REFERENCE}

# every symbol include/aqua_learner.h declares (tests/test_learner_cpu.py checks the library exports them all)
SYMBOLS = ("aqualrn_version", "aqualrn_last_error", "aqualrn_workspace_bytes", "aqualrn_update_f32")


class AquaLearnerError(RuntimeError):
    pass


_vp, _i64, _u64, _ci, _cd, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
_SIGNATURES = {
    "aqualrn_workspace_bytes": ([_i64], _sz),
    "aqualrn_update_f32": ([_vp, _vp, _vp, _vp, _vp,                        # theta, theta_target, m, v, t
                            _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,       # s, a, r, s2, d, ok, ld, size
                            _vp, _i64, _u64,                                # idx, B, seed
                            _ci, _cd, _cd, _cd, _cd, _cd, _cd,              # strategy, gamma, tau, lr, beta1, beta2, eps
                            _vp, _vp, _vp, _i64,                            # blob_online, blob_target, perm, blob_floats
                            _vp, _sz,                                       # workspace, workspace_bytes
                            _vp, _vp, _vp, _vp], _ci),                      # idx_out, grad_out, loss, stream
}

lib = _loader.load("libaqua_learner.so", LIB_PATH, "aqualrn", ABI_VERSION, _SIGNATURES)
check = _loader.checker(lib, "aqualrn", AquaLearnerError)


def flatten(layers):
    """[(kernel [in, out], bias [out])] * 3 -> the canonical float32 parameter vector [PARAMS]"""
    import numpy as np
    layers = list(layers)
    if len(layers) != 3:
        raise ValueError("the Q-network has three dense layers, got %d" % len(layers))
    parts = []
    for (k, b), shape in zip(layers, ((5, 64), (64, 64), (64, 3))):
        k, b = np.asarray(k, dtype=np.float32), np.asarray(b, dtype=np.float32).reshape(-1)
        if k.shape != shape or b.shape != (shape[1],):
            raise ValueError("kernel %s / bias %s: the network is 5-64-64-3 (main/impl/dqn.py:301-314)" % (k.shape, b.shape))
        parts += [k.reshape(-1), b]
    return np.concatenate(parts)


def unflatten(theta):
    """the canonical parameter vector -> layer list as tf_import.dense_stack() returns it (copies)"""
    import numpy as np
    theta = np.asarray(theta, dtype=np.float32).reshape(-1)
    if theta.shape[0] != PARAMS:
        raise ValueError("expected %d parameters, got %d" % (PARAMS, theta.shape[0]))
    out, at = [], 0
    for i, o in ((5, 64), (64, 64), (64, 3)):
        k = theta[at:at + i * o].reshape(i, o).copy()
        at += i * o
        out.append((k, theta[at:at + o].copy()))
        at += o
    return out


def permutation():
    """int32 [PARAMS]: the float index of every parameter in the device-format blob of aqua_policy.h, found by packing
    the values 1..PARAMS (packing is a pure permutation; every other blob float is zero)"""
    import numpy as np
    from . import _policy_capi
    blob = _policy_capi.pack_weights(unflatten(np.arange(1, PARAMS + 1, dtype=np.float32))).view(np.float32)
    at = np.nonzero(blob)[0]
    perm = np.full(PARAMS, -1, dtype=np.int32)
    perm[blob[at].astype(np.int64) - 1] = at.astype(np.int32)
    if at.shape[0] != PARAMS or (perm < 0).any():
        raise AquaLearnerError("aquapol_pack_weights is not a permutation of the %d parameters" % PARAMS)
    return perm
