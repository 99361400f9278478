"""QEnsemble: the networks of a QNetworkBank acting TOGETHER -- libaqua_ens.so (csrc/aqua_ens.h): every member network
evaluates every world of the batch, and one launch reduces the answers to one action per world, by the mean of Q
(mode="mean") or by majority vote (mode="vote"), optionally with the across-network variance of Q and the vote counts
(DESIGN.md 5.20).  What a population is usually for once it is trained: a better policy than its best member, and an
uncertainty signal.

A QEnsemble is a policy wherever a QNetwork or a QNetworkBank is one: act(), q_values(), env.step(policy=ens),
env.rollout(steps, actions=ens), env.capture_policy_step(ens), episodes.evaluate(env, ens).  It reads the bank's own
memory with no copy: a load(), a learner update or a selection is seen by the next launch or graph replay.  With one
member it is that member's QNetwork, bit for bit, epsilon-greedy draws included.

An ensemble is a policy, not a network to train: it has no `blob`, no `tensor` and no `layers` (asking raises TypeError);
DQNLearner, DQNLoop and FastActor take bank.view(p) or the bank.  There is no CPU path.
"""
from . import _ens_capi, _policy_capi
from .qpolicy import QNetwork


class QEnsemble(QNetwork):
    _aquapol_network = True           # what BatchedAqua looks for in step(policy=...) / rollout(actions=...)

    def __init__(self, bank, members=None, mode="mean"):
        """bank: a QNetworkBank.  members: None (every slot); a sequence of slot indices, of which the mask tensor is built
        once; or a contiguous uint8 [>= networks] tensor on the bank's device, owned by the caller, read when the kernel
        runs (it may be rewritten between launches, or by a node of a graph): slot p is a member iff mask[p] != 0.
        mode: "mean" or "vote".  Anything else: ValueError."""
        if not (getattr(bank, "_aquapol_network", False) and hasattr(bank, "networks") and hasattr(bank, "seg") and hasattr(bank, "view")):
            raise ValueError("expected a QNetworkBank")
        if mode not in _ens_capi.MODES:
            raise ValueError("mode %r: one of %s" % (mode, sorted(_ens_capi.MODES)))
        torch = bank.torch
        self.torch, self.device = torch, bank.device
        self.bank, self.mode = bank, mode
        self.networks = int(bank.networks)
        self._bank = bank.tensor                           # the bank's own memory, uint8 [networks][bytes of a slot]: no copy
        if self._bank.dtype != torch.uint8 or int(self._bank.numel()) != self.networks * int(_ens_capi.lib.aquaens_weights_bytes()) \
                or not self._bank.is_contiguous() \
                or int(_ens_capi.lib.aquaens_weights_bytes()) != int(_policy_capi.lib.aquapol_weights_bytes()):
            raise RuntimeError("libaqua_ens.so and libaqua_policy.so disagree on the blob: rebuild")
        if members is None:
            self.mask = None
        elif isinstance(members, torch.Tensor):
            if members.dtype != torch.uint8 or members.device != self.device or members.dim() != 1 or members.numel() < self.networks \
                    or not members.is_contiguous():
                raise ValueError("members must be a contiguous uint8 [>=%d] tensor on %s" % (self.networks, self.device))
            self.mask = members
        elif isinstance(members, (list, tuple, range)) or (hasattr(members, "__iter__") and not isinstance(members, (str, bytes, dict))):
            host = torch.zeros(self.networks, dtype=torch.uint8)
            for p in members:
                if isinstance(p, bool) or int(p) != p or not 0 <= int(p) < self.networks:
                    raise ValueError("member %r: a slot index in [0, %d)" % (p, self.networks))
                host[int(p)] = 1
            self.mask = host.to(self.device)
        else:
            raise ValueError("members must be None, a sequence of slot indices or a uint8 tensor on the device")
        self._epsilon = None
        self._variance = self._votes = None
        self._x_ld = self._x_cols = 0
        self.last_error = ""

    # ------------------------------------------------------------------ what an ensemble is not
    def _not_a_network(self):
        raise TypeError("a QEnsemble acts with the networks of its bank and holds no weights of its own: train bank.view(p)")

    @property
    def blob(self):
        self._not_a_network()

    @property
    def tensor(self):
        self._not_a_network()

    @property
    def layers(self):
        self._not_a_network()

    def load(self, layers):
        self._not_a_network()

    # ------------------------------------------------------------------ plumbing
    @property
    def epsilon(self):
        """None: the ensemble explores with the epsilon of the call.  A float32 [1] tensor on the device, owned by the
        caller: it replaces the epsilon of the call, read when the kernel runs (NaN or negative: never explores)."""
        return self._epsilon

    @epsilon.setter
    def epsilon(self, t):
        torch = self.torch
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or t.numel() != 1
                              or not t.is_contiguous()):
            raise ValueError("epsilon must be None or a float32 [1] tensor on %s" % (self.device,))
        self._epsilon = t

    def attach(self, variance=None, votes=None):
        """variance: float32 [3][x_ld], votes: int32 [3][x_ld] on the device (or None): every following launch also fills
        their first n columns with the across-member population variance of Q and the vote counts.  Both given: the same
        row stride.  A launch with more worlds than they hold raises before it is queued; nothing is allocated in a launch."""
        torch = self.torch
        strides = []
        for t, dtype, what in ((variance, torch.float32, "variance"), (votes, torch.int32, "votes")):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or t.dim() != 2 or t.shape[0] != 3 \
                    or t.stride(1) != 1 or t.shape[1] < 1 or t.stride(0) < t.shape[1]:
                raise ValueError("%s must be a %s [3][x_ld] tensor with unit inner stride on %s" % (what, str(dtype).split(".")[-1], self.device))
            strides.append((int(t.stride(0)), int(t.shape[1])))
        if len(strides) == 2 and strides[0][0] != strides[1][0]:
            raise ValueError("variance and votes must have the same row stride, got %d and %d" % (strides[0][0], strides[1][0]))
        self._variance, self._votes = variance, votes
        self._x_ld = strides[0][0] if strides else 0
        self._x_cols = min(s[1] for s in strides) if strides else 0
        return self

    def launch(self, in_ptr, ld, normalised, n, env_offset, epsilon, seed, tick, tick_base_ptr, action_ptr, q_ptr, q_ld,
               q_taken_ptr, stream):
        """aquaens_act_f32 on raw pointers, QNetwork.launch's signature -> return code.  BatchedAqua turns a non-zero code
        into an exception with the policy library's checker; this library's own message is kept in last_error."""
        var, votes = self._variance, self._votes
        if (var is not None or votes is not None) and n > self._x_cols:
            self.last_error = ""                           # (the message travels with the exception, not with a return code)
            raise ValueError("aquaens_act_f32: n=%d worlds: the attached variance / votes hold %d" % (n, self._x_cols))
        eps, mask = self._epsilon, self.mask
        rc = _ens_capi.lib.aquaens_act_f32(self._bank.data_ptr(), self.networks, None if mask is None else mask.data_ptr(),
                                           _ens_capi.MODES[self.mode], in_ptr, ld, int(bool(normalised)), n, env_offset,
                                           float(epsilon), None if eps is None else eps.data_ptr(),
                                           int(seed) & ((1 << 64) - 1), int(tick) & ((1 << 64) - 1), tick_base_ptr, action_ptr,
                                           q_ptr, q_ld, q_taken_ptr, None if var is None else var.data_ptr(),
                                           None if votes is None else votes.data_ptr(), self._x_ld, stream)
        self.last_error = "" if rc == 0 else _ens_capi.last_error()
        return rc

    def _reraise(self, e):
        if self.last_error:
            raise type(e)("aquaens_act_f32: %s" % self.last_error) from None
        raise e

    # ------------------------------------------------------------------ the path
    def act(self, env_or_buffer, epsilon=0.0, **kw):
        """QNetwork.act() for the ensemble: every world acts on what the members say together (q receives the mean of
        their Q-values, q_taken the mean of the action taken); self.epsilon, when set, replaces `epsilon`.
        -> the action tensor [n]"""
        self.last_error = ""
        try:
            return QNetwork.act(self, env_or_buffer, epsilon, **kw)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)

    def q_values(self, buffer, n=None, out=None):
        """QNetwork.q_values() for the ensemble: the members' mean Q(s, .) -> float32 [3][n]"""
        self.last_error = ""
        try:
            return QNetwork.q_values(self, buffer, n, out)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)
