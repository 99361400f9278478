"""QNetworkBank: P Q-networks (main/impl/dqn.py:301-314, 5 -> 64 ReLU -> 64 ReLU -> 3) acting on ONE batch in a single
launch of libaqua_bank.so (include/aqua_bank.h): network p takes worlds [p * seg, (p + 1) * seg).  What the reference
does policy by policy -- main/plotting/dqn_test_plotter.py::run_tests over tests_config, the checkpoints a training
writes every 100 episodes (dqn.py:316-321) -- is one BatchedAqua here, with env.step(policy=bank),
env.rollout(steps, actions=bank), env.capture_policy_step(bank) and episodes.evaluate(env, bank).

All slots live in ONE device tensor for the lifetime of the object; slot p is byte for byte the blob of a QNetwork of
the same weights, and per segment the bank writes bit for bit what that QNetwork writes.  bank.view(p) is a QNetwork
over slot p without a copy: view.load() or a DQNLearner(view) change the weights the bank acts with on its next launch or
graph replay.  There is no CPU path.

A bank is a policy, not a network to train: it shares QNetwork's act() / q_values() plumbing, but its `layers` is a list of
layer stacks and it has no `blob` (asking for it raises).  DQNLearner and DQNLoop take bank.view(p).
"""
import numpy as np

from . import _bank_capi, _policy_capi
from .qpolicy import QNetwork


class _Slot(QNetwork):
    """QNetwork over one slot of a bank: the same launch, act(), q_values() and load(), on the bank's memory."""

    def __init__(self, bank, p):
        self.torch, self.device = bank.torch, bank.device
        self.bank, self.index = bank, p
        self._blob = bank.tensor[p]

    @property
    def layers(self):
        return self.bank.layers[self.index]

    @layers.setter
    def layers(self, layers):
        if layers is not None:
            self.bank.layers[self.index] = layers

    def weights(self):
        """the slot read back from the device through aquabank_unpack_weights (a host read); also refreshes layers"""
        self.layers = _bank_capi.unpack_weights(self._blob.cpu().numpy())
        return self.layers


class QNetworkBank(QNetwork):
    _aquapol_network = True           # what BatchedAqua looks for in step(policy=...) / rollout(actions=...)

    def __init__(self, networks, worlds_per_network, device=None):
        """networks: a list of layer stacks, each [(kernel [in, out], bias [out])] * 3 as tf_import.dense_stack() returns
        them; worlds_per_network: seg, the worlds each network acts on (local world i of a launch goes to network i // seg)."""
        import torch
        self.torch = torch
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("QNetworkBank runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (device,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: QNetworkBank has no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        networks = list(networks)
        if not 1 <= len(networks) <= _bank_capi.MAX_NETWORKS:
            raise ValueError("a bank holds 1 .. %d networks, got %d" % (_bank_capi.MAX_NETWORKS, len(networks)))
        if int(worlds_per_network) < 1:
            raise ValueError("worlds_per_network=%r: must be >= 1" % (worlds_per_network,))
        self.networks, self.seg = len(networks), int(worlds_per_network)
        slot = int(_bank_capi.lib.aquabank_weights_bytes())
        if slot != int(_policy_capi.lib.aquapol_weights_bytes()):
            raise RuntimeError("libaqua_bank.so and libaqua_policy.so disagree on the blob: rebuild")
        host = np.stack([_policy_capi.pack_weights(layers) for layers in networks])
        self.layers = [[(np.array(k, dtype=np.float32, copy=True), np.array(b, dtype=np.float32, copy=True)) for k, b in layers]
                       for layers in networks]
        self._blob = torch.zeros((self.networks, slot), dtype=torch.uint8, device=dev)
        self._blob.copy_(torch.from_numpy(host))
        self._epsilon = None
        self.last_error = ""

    # ------------------------------------------------------------------ plumbing
    @property
    def tensor(self):
        """the bank: uint8 [networks][aquabank_weights_bytes()] on the device, row p the blob of network p"""
        return self._blob

    @property
    def blob(self):
        """a bank has no single blob: what re-packs into one (DQNLearner, DQNLoop) takes a slot, bank.view(p)"""
        raise TypeError("a QNetworkBank holds %d blobs (bank.tensor): pass bank.view(p) where one QNetwork is wanted" % self.networks)

    @classmethod
    def from_saved_model(cls, variables_dirs, worlds_per_network, device=None):
        """The variables/ directories of Keras SavedModels written by dqn.py:316-321, one per slot, read without TensorFlow."""
        from .tf_import import read_checkpoint, dense_stack
        return cls([dense_stack(read_checkpoint(d)) for d in variables_dirs], worlds_per_network, device)

    @property
    def epsilon(self):
        """None: every network explores with the epsilon of the call.  A float32 [>= networks] tensor on the device, owned
        by the caller: network p explores with epsilon[p], read when the kernel runs (NaN or negative: never)."""
        return self._epsilon

    @epsilon.setter
    def epsilon(self, t):
        torch = self.torch
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or t.dim() != 1
                              or t.numel() < self.networks or not t.is_contiguous()):
            raise ValueError("epsilon must be None or a contiguous float32 [>=%d] tensor on %s" % (self.networks, self.device))
        self._epsilon = t

    def view(self, p):
        """a QNetwork over slot p, no copy: torch, device, layers, blob, load(), launch(), act(), q_values(), weights()"""
        p = int(p)
        if not 0 <= p < self.networks:
            raise IndexError("slot %d of a bank of %d" % (p, self.networks))
        return _Slot(self, p)

    def load(self, networks):
        """Replace every network: packed on the host, copied into the SAME device tensor on the current stream."""
        networks = list(networks)
        if len(networks) != self.networks:
            raise ValueError("the bank holds %d networks, got %d" % (self.networks, len(networks)))
        for p, layers in enumerate(networks):
            self.view(p).load(layers)
        return self

    def split(self, x):
        """a per-world result (tensor or array whose last axis holds networks * seg worlds) -> [..., networks, seg]"""
        n = self.networks * self.seg
        if x.shape[-1] != n:
            raise ValueError("expected %d = %d x %d worlds on the last axis, got %d" % (n, self.networks, self.seg, x.shape[-1]))
        return x.reshape(tuple(x.shape[:-1]) + (self.networks, self.seg))

    def launch(self, in_ptr, ld, normalised, n, env_offset, epsilon, seed, tick, tick_base_ptr, action_ptr, q_ptr, q_ld,
               q_taken_ptr, stream):
        """aquabank_act_f32 on raw pointers, QNetwork.launch's signature -> return code.  BatchedAqua turns a non-zero code
        into an exception with the policy library's checker; the bank's own message is kept in last_error."""
        eps = self._epsilon
        rc = _bank_capi.lib.aquabank_act_f32(self._blob.data_ptr(), self.networks, self.seg, in_ptr, ld, int(bool(normalised)), n,
                                             env_offset, float(epsilon), None if eps is None else eps.data_ptr(),
                                             int(seed) & ((1 << 64) - 1), int(tick) & ((1 << 64) - 1), tick_base_ptr, action_ptr,
                                             q_ptr, q_ld, q_taken_ptr, stream)
        self.last_error = "" if rc == 0 else _bank_capi.last_error()
        return rc

    def _reraise(self, e):
        if self.last_error:
            raise type(e)("aquabank_act_f32: %s" % self.last_error) from None
        raise e

    # ------------------------------------------------------------------ the path
    def act(self, env_or_buffer, epsilon=0.0, **kw):
        """QNetwork.act() for the bank: world i of the batch acts with network i // seg; self.epsilon, when set, replaces
        `epsilon` per network.  -> the action tensor [n]"""
        self.last_error = ""
        try:
            return QNetwork.act(self, env_or_buffer, epsilon, **kw)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)

    def q_values(self, buffer, n=None, out=None):
        """QNetwork.q_values() for the bank: Q(s, .) of column i under network i // seg -> float32 [3][n]"""
        self.last_error = ""
        try:
            return QNetwork.q_values(self, buffer, n, out)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)
