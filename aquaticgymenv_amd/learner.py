"""DQNLearner: the reference's training step (main/impl/dqn.py:175-176: the "double" target as dqn.py:262-272 executes
it, a squared-error loss, Keras 2.3's Adam of dqn.py:313, the soft target update of dqn.py:294-299) for a minibatch of a
ReplayRing, on the device by libaqua_learner.so (include/aqua_learner.h).

The loss has three forms (T_bj = y_b for j = a_b and Q(s_b)[j] otherwise, held constant):
  loss="reference"  what the reference's default "custom_grad" step executes: dqn.py:244 keeps the prediction [B,1],
                    dqn.py:246 subtracts the whole [B,3] target array, the difference broadcasts and dqn.py:247 averages
                    3 B elements: L = 1/(3B) sum_b sum_j (Q_a - T_bj)^2, gradient 2/(3B) (3 Q_a - y - sum_{j != a} Q_j).
  (not offered)     its "standard" step, train_on_batch with Keras "mse" (dqn.py:236, 313): 1/(3B) sum_b (Q_a - y)^2, the
                    textbook direction with a factor 1/3.
  loss="mse"        the default here: the textbook 1/B sum_b (Q_a - y)^2, gradient 2/B_eff (Q_a - y) -- neither of the
                    reference's paths exactly; it differs from "reference" in direction, not only in scale.

Two launches per update, no allocation, no synchronisation, no host read: update() works unchanged inside
torch.cuda.graph.  The new weights are scattered into the acting QNetwork's device blob, so env.step(policy=qnet) and a
captured capture_policy_step(qnet) act with them on their next launch.  float32 forward and backward (the last layer and
the TD error in double), bit-reproducible for the same inputs.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _learner_capi


class DQNLearner(object):
    BETA1, BETA2, EPS = 0.9, 0.999, 1e-7          # tf.keras.optimizers.Adam's defaults (dqn.py:313)

    def __init__(self, qnet, gamma=0.98, tau=0.005, lr=1e-3, strategy="double_ref", seed=0, loss="mse"):
        """qnet: the acting QNetwork; theta and theta_target start from qnet.layers.  gamma, tau, lr: default_hyperparam's.
        strategy: "double_ref" (what dqn.py:267-268 executes), "double" (what its comment says), "fixed", "standard".
        loss: "mse" (the mean squared TD error) or "reference" (the broadcast dqn.py:243-247 executes), see above."""
        if not getattr(qnet, "_aquapol_network", False):
            raise ValueError("expected a QNetwork")
        if strategy not in _learner_capi.STRATEGIES:
            raise ValueError("strategy %r: one of %s" % (strategy, sorted(_learner_capi.STRATEGIES)))
        if loss not in _learner_capi.LOSSES:
            raise ValueError("loss %r: one of %s" % (loss, sorted(_learner_capi.LOSSES)))
        torch = qnet.torch
        self.torch = torch
        self.qnet = qnet
        self.device = qnet.device
        self.gamma, self.tau, self.lr = float(gamma), float(tau), float(lr)
        self.beta1, self.beta2, self.eps = self.BETA1, self.BETA2, self.EPS
        self.strategy = strategy
        self.loss_form = loss
        self.seed = int(seed) & ((1 << 64) - 1)
        dev = self.device
        n = _learner_capi.PARAMS
        theta = torch.from_numpy(_learner_capi.flatten(qnet.layers)).to(dev)
        self.theta = theta.clone()
        self.theta_target = theta.clone()
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.perm = torch.from_numpy(_learner_capi.permutation()).to(dev)
        # the target network in the acting network's format (QNetwork.q_values-compatible): re-packed by every update
        self.target_blob = qnet.blob.clone()
        self._workspace = None
        self._grow(64)

    # ------------------------------------------------------------------ plumbing
    def _grow(self, batch_size):
        need = int(_learner_capi.lib.aqualrn_workspace_bytes(int(batch_size)))
        if need == 0:
            raise ValueError("batch_size=%d: must be in [0, %d]" % (batch_size, _learner_capi.MAX_BATCH))
        if self._workspace is None or self._workspace.numel() < need:
            if self.torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the workspace must grow outside of a graph capture: run one update of this batch size first")
            self._workspace = self.torch.zeros(need, dtype=self.torch.uint8, device=self.device)
        return need

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ the path
    def update(self, ring, batch_size=64, idx=None, idx_out=None, gamma=None):
        """One update from `ring` (a ReplayRing of discrete actions, or anything with its s, a, r, s2, d, ok tensors,
        capacity and size), queued on torch's current stream of the ring's device.
        idx: int32 [batch_size] (or [1][batch_size], one network's row of a bank's draw) slots; None: drawn on the device (Philox stream 6, keyed by seed, the sample number and the
        update number).  A slot outside [0, ring.size) or with ok == 0 is not a sample.  idx_out: optional int32
        [batch_size] receiving the slot used (-1: none).  The loss before the update is left in self.loss, the gradient in
        self.grad.  gamma: None, or the discount of THIS call in place of self.gamma -- gamma^n with the staged rows of an
        NStepReturns (nstep.py), whose idx is int32 [1][batch_size].  -> self.loss"""
        torch = self.torch
        if ring.a.dtype != torch.uint8 or ring.a.dim() != 1:
            raise ValueError("the Q-network (main/impl/dqn.py) is defined for discrete actions: the ring holds continuous ones")
        if ring.s.device != self.device:
            raise ValueError("the ring is on %s, the learner on %s" % (ring.s.device, self.device))
        B = int(batch_size)
        cap = int(ring.capacity)
        for name, rows, dtype in (("s", 5, torch.float32), ("s2", 5, torch.float32), ("r", 1, torch.float32), ("a", 1, torch.uint8),
                                  ("d", 1, torch.uint8), ("ok", 1, torch.uint8)):
            t = getattr(ring, name)
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != rows * cap:
                raise ValueError("ring.%s must be a contiguous %s tensor of %d x %d" % (name, dtype, rows, cap))
        for name, t in (("idx", idx), ("idx_out", idx_out)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device
                                  or not (t.dim() == 1 or (name == "idx" and t.dim() == 2 and t.shape[0] == 1))
                                  or t.numel() < B or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous int32 [>=%d]%s tensor on %s"
                                 % (name, B, " or [1][>=%d]" % B if name == "idx" else "", self.device))
        need = self._grow(B)
        with torch.cuda.device(self.device):
            rc = _learner_capi.lib.aqualrn_update_f32(
                self.theta.data_ptr(), self.theta_target.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.t.data_ptr(),
                ring.s.data_ptr(), ring.a.data_ptr(), ring.r.data_ptr(), ring.s2.data_ptr(), ring.d.data_ptr(),
                ring.ok.data_ptr(), cap, int(ring.size),
                None if idx is None else idx.data_ptr(), B, self.seed,
                _learner_capi.STRATEGIES[self.strategy] | _learner_capi.LOSSES[self.loss_form], self.gamma if gamma is None else float(gamma), self.tau, self.lr, self.beta1, self.beta2, self.eps,
                self.qnet.blob.data_ptr(), self.target_blob.data_ptr(), self.perm.data_ptr(), self.qnet.blob.numel() // 4,
                self._workspace.data_ptr(), need,
                None if idx_out is None else idx_out.data_ptr(), self.grad.data_ptr(), self.loss.data_ptr(), self._stream())
        _learner_capi.check(rc, "aqualrn_update_f32")
        return self.loss

    # ------------------------------------------------------------------ reading and resuming
    def weights(self):
        """the online network as tf_import.dense_stack() returns it (a host read); also refreshes qnet.layers"""
        layers = _learner_capi.unflatten(self.theta.cpu().numpy())
        self.qnet.layers = [(k.copy(), b.copy()) for k, b in layers]
        return layers

    def target_weights(self):
        return _learner_capi.unflatten(self.theta_target.cpu().numpy())

    def state_dict(self):
        out = {name: getattr(self, name).detach().cpu().clone() for name in ("theta", "theta_target", "m", "v", "t")}
        out["hyper"] = {"gamma": self.gamma, "tau": self.tau, "lr": self.lr, "beta1": self.beta1, "beta2": self.beta2,
                        "eps": self.eps, "strategy": self.strategy, "seed": self.seed, "loss": self.loss_form}
        return out

    def load_state_dict(self, state):
        """Resume bit for bit: parameters, Adam's moments, the update counter (the key of the next minibatch draw), the
        hyper-parameters; the acting network's blob and the target blob are re-packed."""
        from . import _policy_capi
        torch = self.torch
        for name in ("theta", "theta_target", "m", "v", "t"):
            src = torch.as_tensor(state[name])
            dst = getattr(self, name)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name, dst.dtype, tuple(dst.shape)))
            dst.copy_(src)
        h = state.get("hyper", {})
        if h.get("strategy", self.strategy) not in _learner_capi.STRATEGIES:
            raise ValueError("strategy %r" % (h["strategy"],))
        if h.get("loss", "mse") not in _learner_capi.LOSSES:
            raise ValueError("loss %r" % (h["loss"],))
        for key in ("gamma", "tau", "lr", "beta1", "beta2", "eps", "strategy", "seed"):
            if key in h:
                setattr(self, key, h[key])
        if "hyper" in state:
            self.loss_form = h.get("loss", "mse")            # absent in checkpoints written before the option existed
        self.qnet.load(_learner_capi.unflatten(np.asarray(state["theta"])))
        self.target_blob.copy_(torch.from_numpy(_policy_capi.pack_weights(_learner_capi.unflatten(np.asarray(state["theta_target"])))))
        return self
