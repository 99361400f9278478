"""QNetwork: the reference's DQN model (main/impl/dqn.py:301-314, 5 -> 64 ReLU -> 64 ReLU -> 3) evaluated on the device
by libaqua_policy.so (include/aqua_policy.h) -- greedy for evaluation (main/testing/test_dqn.py:14-22), epsilon-greedy
for training (dqn.py:212-228), Q-values out for TD targets (dqn.py:262-292).

One launch per batch, activations in registers; float32 throughout.  The weights live in ONE device blob for the
lifetime of the object: load() re-packs into it, so a graph captured with this network acts with the new weights on its
next replay.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _policy_capi


class QNetwork(object):
    _aquapol_network = True           # what BatchedAqua looks for in step(policy=...) / rollout(actions=...)

    def __init__(self, layers, device=None):
        """layers: [(kernel [in, out], bias [out])] * 3, numpy arrays as tf_import.dense_stack() returns them."""
        import torch
        self.torch = torch
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("QNetwork runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (device,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: QNetwork has no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._blob = torch.zeros(int(_policy_capi.lib.aquapol_weights_bytes()), dtype=torch.uint8, device=dev)
        self.layers = None
        self.load(layers)

    @classmethod
    def from_saved_model(cls, variables_dir, device=None):
        """The variables/ directory of a Keras SavedModel written by dqn.py:316-321, read without TensorFlow."""
        from .tf_import import read_checkpoint, dense_stack
        return cls(dense_stack(read_checkpoint(variables_dir)), device)

    def load(self, layers):
        """Replace the weights: packed on the host, copied into the SAME device blob on the current stream."""
        blob = _policy_capi.pack_weights(layers)
        self.layers = [(np.array(k, dtype=np.float32, copy=True), np.array(b, dtype=np.float32, copy=True)) for k, b in layers]
        self._blob.copy_(self.torch.from_numpy(blob))
        return self

    # ------------------------------------------------------------------ plumbing
    @property
    def blob(self):
        """the device-format weights (uint8, aquapol_weights_bytes()): what DQNLearner re-packs into after every update"""
        return self._blob

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def launch(self, in_ptr, ld, normalised, n, env_offset, epsilon, seed, tick, tick_base_ptr, action_ptr, q_ptr, q_ld,
               q_taken_ptr, stream):
        """aquapol_act_f32 on raw pointers -> return code (callers that capture graphs check it themselves)."""
        return _policy_capi.lib.aquapol_act_f32(self._blob.data_ptr(), in_ptr, ld, int(bool(normalised)), n, env_offset,
                                                float(epsilon), int(seed) & ((1 << 64) - 1), int(tick) & ((1 << 64) - 1),
                                                tick_base_ptr, action_ptr, q_ptr, q_ld, q_taken_ptr, stream)

    def _f32(self, t, rows, n, what):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device:
            raise ValueError("%s must be a float32 tensor on %s" % (what, self.device))
        if rows == 1:
            if t.dim() != 1 or t.numel() < n or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float32 [>=%d] tensor" % (what, n))
            return t.data_ptr(), t.numel()
        if t.dim() != 2 or t.shape[0] < rows or t.shape[1] < n or t.stride(1) != 1:
            raise ValueError("%s must be float32 [>=%d][>=%d] with unit inner stride" % (what, rows, n))
        return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1])

    # ------------------------------------------------------------------ the path
    def act(self, env_or_buffer, epsilon=0.0, out=None, q=None, q_taken=None, normalised=None, n=None, env_offset=None,
            seed=None, tick=None, tick_base=None):
        """Actions (and Q-values) for a batch.

        env_or_buffer: a BatchedAqua -- its state rows are read and normalised in the kernel (normalised=True: its obs_norm
                       buffer is read instead; the result is the same bit for bit); world range, seed and the tick of the step
                       about to be taken come from it --
                       or a float32 [5][ld] tensor holding the network's input (ReplayRing.s / .s2, env.obs_norm_buf;
                       normalised=False: [>=5][ld] state rows), with n worlds (default: all columns).
        epsilon:       0 greedy (lowest index on a tie); > 0 explores with probability epsilon, keyed by
                       (seed, env_offset + world, tick [+ tick_base[0] on the device], Philox stream 5).
        out:           uint8 [>=n] for the actions (default: a new tensor); q: float32 [3][>=n]; q_taken: float32 [>=n].
        -> the action tensor [n]."""
        torch = self.torch
        if hasattr(env_or_buffer, "state") and hasattr(env_or_buffer, "num_envs"):
            env = env_or_buffer
            if env.continuous:
                raise ValueError("the Q-network (main/impl/dqn.py) is defined for discrete actions")
            if env.device != self.device:
                raise ValueError("the environment is on %s, the network on %s" % (env.device, self.device))
            buf = env.obs_norm_buf if normalised else env.state
            if buf is None:
                raise RuntimeError("normalised=True: construct the env with normalized_obs=True")
            normalised = bool(normalised)
            n = env.num_envs if n is None else int(n)
            env_offset = env.env_offset if env_offset is None else env_offset
            seed = env.seed if seed is None else seed
            tick = env._tick if tick is None else tick
        else:
            buf = env_or_buffer
            normalised = True if normalised is None else bool(normalised)
            if not isinstance(buf, torch.Tensor) or buf.dim() != 2:
                raise ValueError("expected a BatchedAqua or a float32 [5][ld] tensor")
            n = buf.shape[1] if n is None else int(n)
            env_offset, seed, tick = env_offset or 0, seed or 0, tick or 0
        in_ptr, ld = self._f32(buf, 5, n, "the input")
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != self.device or out.dim() != 1 \
                or out.numel() < n or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 [>=%d] tensor on %s" % (n, self.device))
        q_ptr, q_ld = self._f32(q, 3, n, "q") if q is not None else (None, 0)
        qt_ptr = self._f32(q_taken, 1, n, "q_taken")[0] if q_taken is not None else None
        tb_ptr = None
        if tick_base is not None:
            if tick_base.dtype != torch.int64 or tick_base.device != self.device or tick_base.numel() < 1:
                raise ValueError("tick_base must be an int64 tensor on %s" % (self.device,))
            tb_ptr = tick_base.data_ptr()
        with torch.cuda.device(self.device):
            _policy_capi.check(self.launch(in_ptr, ld, normalised, n, env_offset, epsilon, seed, tick, tb_ptr, out.data_ptr(),
                                           q_ptr, q_ld, qt_ptr, self._stream()), "aquapol_act_f32")
        return out[:n]

    def q_values(self, buffer, n=None, out=None):
        """Q(s, .) of a float32 [5][ld] buffer of normalised observations (ReplayRing.s / .s2) -> float32 [3][n];
        dqn.py:262-292 takes its arg-max / max / gather from this with one torch reduction."""
        torch = self.torch
        if not isinstance(buffer, torch.Tensor) or buffer.dim() != 2:
            raise ValueError("expected a float32 [5][ld] tensor")
        n = buffer.shape[1] if n is None else int(n)
        in_ptr, ld = self._f32(buffer, 5, n, "the input")
        if out is None:
            out = torch.empty((3, max(n, 1)), dtype=torch.float32, device=self.device)
        q_ptr, q_ld = self._f32(out, 3, n, "out")
        with torch.cuda.device(self.device):
            _policy_capi.check(self.launch(in_ptr, ld, True, n, 0, 0.0, 0, 0, None, None, q_ptr, q_ld, None, self._stream()),
                               "aquapol_act_f32")
        return out[:, :n]
