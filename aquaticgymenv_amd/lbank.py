"""DQNLearnerBank: the training half of a QNetworkBank.  Every network of the bank takes one DQNLearner update (learner.py:
TD target, gradient, Adam, soft target update, re-pack into the acting blob) from a minibatch of its OWN transitions in
the ONE experience ring of the batch, in two launches of libaqua_lbank.so (include/aqua_lbank.h) for the whole bank, and
the minibatches of all networks are drawn in one more.

The state of the P learners is stacked -- theta, theta_target, m, v float32 [P][4739], t int64 [P] -- and the acting blobs
are the bank's own tensor, so env.step(policy=bank) acts with the new weights on its next launch or graph replay.  gamma,
tau and lr are per network (a device table the kernels read); the bootstrap strategy and the loss form are the bank's.
Slot p of everything an update writes is bit for bit what DQNLearner(bank.view(p), ...) writes for the same minibatch.

No new ring: DeviceReplayRing places world i of a batch of N worlds in slot base + i, so with a capacity that is a multiple
of N slot s always holds a transition of world s mod N, which network (s mod N) // seg acted in.  draw() confines the
draw of network p to those slots.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _lbank_capi, _learner_capi
from .learner import DQNLearner

_STACKED = ("theta", "theta_target", "m", "v", "t")


def _per_network(value, P, what):
    """a scalar or a sequence of P values -> float64 [P]"""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        return np.full(P, float(a), dtype=np.float64)
    if a.shape != (P,):
        raise ValueError("%s: a scalar or %d values, got shape %s" % (what, P, a.shape))
    return a.copy()


class DQNLearnerBank(object):
    BETA1, BETA2, EPS = DQNLearner.BETA1, DQNLearner.BETA2, DQNLearner.EPS

    def __init__(self, bank, gamma=0.98, tau=0.005, lr=1e-3, strategy="double_ref", loss="mse", seed=0):
        """bank: the acting QNetworkBank; theta and theta_target of slot p start from bank.layers[p].  gamma, tau, lr, seed:
        a scalar or a sequence of P values (a scalar seed s means s + p).  strategy, loss: DQNLearner's, one for the bank."""
        if not hasattr(bank, "networks") or not hasattr(bank, "tensor"):
            raise ValueError("expected a QNetworkBank")
        if strategy not in _learner_capi.STRATEGIES:
            raise ValueError("strategy %r: one of %s" % (strategy, sorted(_learner_capi.STRATEGIES)))
        if loss not in _learner_capi.LOSSES:
            raise ValueError("loss %r: one of %s" % (loss, sorted(_learner_capi.LOSSES)))
        P = int(bank.networks)
        if not 1 <= P <= _lbank_capi.MAX_NETWORKS:
            raise ValueError("a learner bank trains 1 .. %d networks, the bank holds %d" % (_lbank_capi.MAX_NETWORKS, P))
        torch = bank.torch
        self.torch, self.bank, self.device = torch, bank, bank.device
        self.networks, self.seg = P, int(bank.seg)
        self.strategy, self.loss_form = strategy, loss
        self.beta1, self.beta2, self.eps = self.BETA1, self.BETA2, self.EPS
        self._hyper_host = np.stack([_per_network(gamma, P, "gamma"), _per_network(tau, P, "tau"), _per_network(lr, P, "lr"),
                                     np.full(P, self.beta1), np.full(P, self.beta2), np.full(P, self.eps)], axis=1)
        seeds = np.asarray(seed)
        if seeds.ndim == 0:
            seeds = [int(seed) + p for p in range(P)]
        elif seeds.shape != (P,):
            raise ValueError("seed: a scalar or %d values, got shape %s" % (P, seeds.shape))
        self.seeds = [int(s) & ((1 << 64) - 1) for s in seeds]
        dev, n = self.device, _lbank_capi.PARAMS
        self.blob_floats = bank.tensor.shape[1] // 4
        theta = torch.from_numpy(np.stack([_learner_capi.flatten(layers) for layers in bank.layers])).to(dev)
        self.theta = theta.clone()
        self.theta_target = theta.clone()
        self.m = torch.zeros((P, n), dtype=torch.float32, device=dev)
        self.v = torch.zeros((P, n), dtype=torch.float32, device=dev)
        self.t = torch.zeros(P, dtype=torch.int64, device=dev)
        self.loss = torch.zeros(P, dtype=torch.float32, device=dev)
        self.grad = torch.zeros((P, n), dtype=torch.float32, device=dev)
        self.perm = torch.from_numpy(_learner_capi.permutation()).to(dev)
        # the target networks in the bank's format: row p is QNetwork.q_values-compatible, re-packed by every update
        self.target_tensor = bank.tensor.clone()
        self.seed_dev = torch.from_numpy(np.array(self.seeds, dtype=np.uint64).view(np.int64)).to(dev)
        self.hyper = torch.from_numpy(_lbank_capi.pack_hyper(self._hyper_host)).to(dev)
        self._workspace = None
        self._grow(64)

    # ------------------------------------------------------------------ plumbing
    def _grow(self, batch_size):
        need = int(_lbank_capi.lib.aqualbank_workspace_bytes(self.networks, int(batch_size)))
        if need == 0:
            raise ValueError("batch_size=%d: must be in [0, %d]" % (batch_size, _lbank_capi.MAX_BATCH))
        if self._workspace is None or self._workspace.numel() < need:
            if self.torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the workspace must grow outside of a graph capture: run one update of this batch size first")
            self._workspace = self.torch.zeros(need, dtype=self.torch.uint8, device=self.device)
        return need

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _idx(self, t, B, what):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device or tuple(t.shape) != (self.networks, B) \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous int32 [%d][%d] tensor on %s" % (what, self.networks, B, self.device))
        return t

    def hyper_of(self, p):
        """-> {"gamma", "tau", "lr", "beta1", "beta2", "eps"} of network p (the host copy of its row)"""
        return dict(zip(_lbank_capi.HYPER_FIELDS, (float(x) for x in self._hyper_host[self._slot(p)])))

    def _slot(self, p):
        p = int(p)
        if not 0 <= p < self.networks:
            raise IndexError("network %d of a bank of %d" % (p, self.networks))
        return p

    def set_hyper(self, p, **kw):
        """Replace hyper-parameters of network p (gamma, tau, lr, beta1, beta2, eps): its row is validated, re-packed and
        copied to the device table on the current stream, outside of a capture; a graph reads it on its next replay."""
        p = self._slot(p)
        if self.torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_hyper() copies from the host: call it outside of a graph capture")
        row = self._hyper_host[p].copy()
        for key, value in kw.items():
            if key not in _lbank_capi.HYPER_FIELDS:
                raise ValueError("%r: one of %s" % (key, list(_lbank_capi.HYPER_FIELDS)))
            row[_lbank_capi.HYPER_FIELDS.index(key)] = float(value)
        try:
            packed = _lbank_capi.pack_hyper(row[None, :])
        except ValueError as e:                               # the library names row 0 of what it was given
            raise ValueError("network %d: %s" % (p, str(e).split(": ", 2)[-1])) from None
        self._hyper_host[p] = row
        self.hyper[p].copy_(self.torch.from_numpy(packed[0]))
        return self

    def sync_hyper(self):
        """Read the device table back into the host copy behind hyper_of(), set_hyper() and state_dict() (a host read).
        Only a PopulationSelector (pbt.py) rewrites rows of the device table: after its select() the host copy is stale
        until this is called; its report() and state_dict() call it."""
        if self.torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sync_hyper() reads back to the host: call it outside of a graph capture")
        self._hyper_host = self.hyper.cpu().numpy()[:, :len(_lbank_capi.HYPER_FIELDS)].copy()
        return self

    # ------------------------------------------------------------------ the path
    def draw(self, ring, batch_size=64, out=None):
        """The minibatch of every network's NEXT update, each from its own slots of `ring` (a DeviceReplayRing whose
        capacity is a multiple of its env's num_envs): one launch -> int32 [P][B], -1 where four attempts met no real
        transition (or the network owns no world)."""
        if getattr(ring, "header", None) is None:
            raise ValueError("expected a DeviceReplayRing")
        if ring.device != self.device:
            raise ValueError("the ring is on %s, the learner bank on %s" % (ring.device, self.device))
        B = int(batch_size)
        if B < 0 or B > _lbank_capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [0, %d]" % (B, _lbank_capi.MAX_BATCH))
        if out is None:
            out = self.torch.empty((self.networks, B), dtype=self.torch.int32, device=self.device)
        self._idx(out, B, "out")
        with self.torch.cuda.device(self.device):
            rc = _lbank_capi.lib.aqualbank_draw(ring.header.data_ptr(), ring.ok.data_ptr(), int(ring.capacity), int(ring.env.num_envs),
                                                self.seg, self.networks, self.t.data_ptr(), self.seed_dev.data_ptr(),
                                                out.data_ptr(), B, self._stream())
        _lbank_capi.check(rc, "aqualbank_draw")
        return out

    def update(self, ring, batch_size, idx, idx_out=None, hyper=None):
        """One update of every network from `ring` (ring.learner_view(), or anything with the s, a, r, s2, d, ok tensors,
        capacity and size of a ring of discrete actions), queued on torch's current stream.  idx: int32 [P][batch_size],
        row p the slots of network p's minibatch (draw()); a slot outside [0, ring.size) or with ok == 0 is not a sample.
        idx_out: optional int32 [P][batch_size] receiving the slots used.  hyper: None, or the device table of THIS call in place of
        self.hyper, a float64 tensor of its shape -- NStepReturns.hyper (nstep.py), the table with gamma^n in word 0, with that
        object's staged rows.  Two launches.  -> self.loss [P] (the loss of every
        network before the update; the gradients are left in self.grad)"""
        torch = self.torch
        if ring.a.dtype != torch.uint8 or ring.a.dim() != 1:
            raise ValueError("the Q-network (main/impl/dqn.py) is defined for discrete actions: the ring holds continuous ones")
        if ring.s.device != self.device:
            raise ValueError("the ring is on %s, the learner bank on %s" % (ring.s.device, self.device))
        B = int(batch_size)
        cap = int(ring.capacity)
        for name, rows, dtype in (("s", 5, torch.float32), ("s2", 5, torch.float32), ("r", 1, torch.float32), ("a", 1, torch.uint8),
                                  ("d", 1, torch.uint8), ("ok", 1, torch.uint8)):
            t = getattr(ring, name)
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != rows * cap:
                raise ValueError("ring.%s must be a contiguous %s tensor of %d x %d" % (name, dtype, rows, cap))
        self._idx(idx, B, "idx")
        if idx_out is not None:
            self._idx(idx_out, B, "idx_out")
        if hyper is None:
            hyper = self.hyper
        elif not isinstance(hyper, torch.Tensor) or hyper.dtype != self.hyper.dtype or hyper.device != self.device \
                or hyper.shape != self.hyper.shape or not hyper.is_contiguous():
            raise ValueError("hyper must be a contiguous %s %s tensor on %s" % (self.hyper.dtype, tuple(self.hyper.shape), self.device))
        need = self._grow(B)
        with torch.cuda.device(self.device):
            rc = _lbank_capi.lib.aqualbank_update_f32(
                self.theta.data_ptr(), self.theta_target.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.t.data_ptr(), self.networks,
                ring.s.data_ptr(), ring.a.data_ptr(), ring.r.data_ptr(), ring.s2.data_ptr(), ring.d.data_ptr(), ring.ok.data_ptr(),
                cap, int(ring.size), idx.data_ptr(), B,
                _learner_capi.STRATEGIES[self.strategy] | _learner_capi.LOSSES[self.loss_form], hyper.data_ptr(),
                self.bank.tensor.data_ptr(), self.target_tensor.data_ptr(), self.perm.data_ptr(), self.blob_floats,
                self._workspace.data_ptr(), need,
                None if idx_out is None else idx_out.data_ptr(), self.grad.data_ptr(), self.loss.data_ptr(), self._stream())
        _lbank_capi.check(rc, "aqualbank_update_f32")
        return self.loss

    # ------------------------------------------------------------------ reading and resuming
    def weights(self, p):
        """the online network of slot p as tf_import.dense_stack() returns it (a host read); also refreshes bank.layers[p]"""
        layers = _learner_capi.unflatten(self.theta[self._slot(p)].cpu().numpy())
        self.bank.layers[int(p)] = [(k.copy(), b.copy()) for k, b in layers]
        return layers

    def target_weights(self, p):
        return _learner_capi.unflatten(self.theta_target[self._slot(p)].cpu().numpy())

    def state_dict(self):
        out = {name: getattr(self, name).detach().cpu().clone() for name in _STACKED}
        out["hyper"] = {"table": self._hyper_host.copy(), "seeds": list(self.seeds), "strategy": self.strategy, "loss": self.loss_form,
                        "networks": self.networks}
        return out

    def load_state_dict(self, state):
        """Resume the whole bank bit for bit: parameters, Adam's moments, the update counters (the keys of the next draws),
        the hyper-parameter table and the seeds; the bank's blobs and the target blobs are re-packed."""
        from . import _policy_capi
        torch = self.torch
        h = state.get("hyper", {})
        if h.get("networks", self.networks) != self.networks:
            raise ValueError("the state holds %r networks, this bank %d" % (h.get("networks"), self.networks))
        if h.get("strategy", self.strategy) not in _learner_capi.STRATEGIES:
            raise ValueError("strategy %r" % (h["strategy"],))
        if h.get("loss", self.loss_form) not in _learner_capi.LOSSES:
            raise ValueError("loss %r" % (h["loss"],))
        for name in _STACKED:
            src, dst = torch.as_tensor(state[name]), getattr(self, name)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name, dst.dtype, tuple(dst.shape)))
        table = np.asarray(h.get("table", self._hyper_host), dtype=np.float64)
        if table.shape != self._hyper_host.shape:
            raise ValueError("hyper table: expected %s, got %s" % (self._hyper_host.shape, table.shape))
        packed = _lbank_capi.pack_hyper(table)
        seeds = [int(s) & ((1 << 64) - 1) for s in h.get("seeds", self.seeds)]
        if len(seeds) != self.networks:
            raise ValueError("seeds: expected %d values" % self.networks)
        for name in _STACKED:
            getattr(self, name).copy_(torch.as_tensor(state[name]))
        self._hyper_host, self.seeds = table.copy(), seeds
        self.hyper.copy_(torch.from_numpy(packed))
        self.seed_dev.copy_(torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)))
        self.strategy, self.loss_form = h.get("strategy", self.strategy), h.get("loss", self.loss_form)
        theta, target = np.asarray(state["theta"]), np.asarray(state["theta_target"])
        self.bank.load([_learner_capi.unflatten(theta[p]) for p in range(self.networks)])
        host = np.stack([_policy_capi.pack_weights(_learner_capi.unflatten(target[p])) for p in range(self.networks)])
        self.target_tensor.copy_(torch.from_numpy(host))
        return self

    def slot_state_dict(self, p):
        """the state of network p in DQNLearner.state_dict()'s format: DQNLearner(bank.view(p)).load_state_dict(...) continues
        that member alone, bit for bit"""
        p = self._slot(p)
        out = {name: getattr(self, name)[p].detach().cpu().clone() for name in ("theta", "theta_target", "m", "v")}
        out["t"] = self.t[p:p + 1].detach().cpu().clone()
        out["hyper"] = dict(self.hyper_of(p), strategy=self.strategy, seed=self.seeds[p], loss=self.loss_form)
        return out
