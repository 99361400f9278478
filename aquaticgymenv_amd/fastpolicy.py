"""FastActor: the fast acting path of a QNetwork, a bank slot or a QNetworkBank -- libaqua_fastpol.so
(csrc/aqua_fastpol.h): the two hidden layers of the 5 -> 64 -> 64 -> 3 network (main/impl/dqn.py:301-314) on the f16 MFMA,
every operand split into a high and a low f16 part, three f16 products for one float32 product.

A FastActor is a policy wherever a QNetwork or a QNetworkBank is one: act(), q_values(), env.step(policy=fast),
env.rollout(steps, actions=fast), env.capture_policy_step(fast), episodes.evaluate(env, fast), and the act stage of
DQNLoop / PopulationLoop (actor=fast).  Its Q-values are those of the float32 path to within a few float32 roundings (the
contract is stated in csrc/aqua_fastpol.h and checked in tests/test_fastpol_gpu.py); its epsilon-greedy draws are the
float32 path's exactly.

The weights.  The source keeps its float32 blob(s): load(), the learners' re-pack and the selector's copy write there.
The actor owns the split copy and refresh() queues ONE launch that re-splits every slot on the current stream; the
constructor does it once.  Acting never refreshes by itself, so a captured graph stays deterministic: A STALE ACTOR ACTS
WITH THE WEIGHTS OF ITS LAST refresh().  DQNLoop and PopulationLoop queue the refresh behind the update themselves.
There is no CPU path.
"""
from . import _fastpol_capi, _policy_capi
from .qpolicy import QNetwork


class FastActor(QNetwork):
    _aquapol_network = True           # what BatchedAqua looks for in step(policy=...) / rollout(actions=...)

    def __init__(self, policy, device=None):
        """policy: a QNetwork, a bank.view(p) or a QNetworkBank; or a layer stack [(kernel, bias)] * 3, of which a QNetwork
        is built on `device` first (a CPU device raises as QNetwork does).  Anything else: ValueError."""
        if isinstance(policy, (list, tuple)):
            policy = QNetwork(policy, device)
        if isinstance(policy, FastActor) or not getattr(policy, "_aquapol_network", False):
            raise ValueError("expected a QNetwork, a bank.view(p) or a QNetworkBank")
        self.torch, self.device = policy.torch, policy.device
        self.source = policy
        self._is_bank = hasattr(policy, "networks") and hasattr(policy, "seg")
        # the float32 blob(s) the refresh reads: uint8 [P][bytes], rows of one tensor (a bank) or the one blob
        self._src = policy.tensor if self._is_bank else policy.blob
        P = self.networks
        if int(self._src.numel()) != P * int(_policy_capi.lib.aquapol_weights_bytes()) or not self._src.is_contiguous():
            raise RuntimeError("libaqua_fastpol.so and libaqua_policy.so disagree on the blob: rebuild")
        torch = self.torch
        self._blob = torch.zeros((P, int(_fastpol_capi.lib.aquafast_weights_bytes())), dtype=torch.uint8, device=self.device)
        self._map = torch.from_numpy(_fastpol_capi.blob_map()).to(self.device)
        self.last_error = ""
        self.refresh()

    # ------------------------------------------------------------------ what a bank has, forwarded
    @property
    def networks(self):
        return self.source.networks if self._is_bank else 1

    @property
    def seg(self):
        """worlds per network; one network takes whatever batch comes"""
        return self.source.seg if self._is_bank else (1 << 62)

    @property
    def epsilon(self):
        """the bank's per-network device epsilon array (None for one network, or when the bank has none)"""
        return self.source.epsilon if self._is_bank else None

    @epsilon.setter
    def epsilon(self, t):
        if not self._is_bank:
            raise TypeError("one network explores with the epsilon of the call")
        self.source.epsilon = t

    def split(self, x):
        if not self._is_bank:
            raise TypeError("one network has no segments to split a result into")
        return self.source.split(x)

    @property
    def layers(self):
        return self.source.layers

    # ------------------------------------------------------------------ the weights
    @property
    def tensor(self):
        """the fast blobs: uint8 [networks][aquafast_weights_bytes()] on the device, as of the last refresh()"""
        return self._blob

    @property
    def blob(self):
        """a learner trains the float32 network: pass the source, not its actor"""
        raise TypeError("a FastActor holds the split copy of its source's weights: pass actor.source where a QNetwork is trained")

    def refresh(self):
        """Queue the re-split of every slot from the source's float32 blob(s) on the current stream: one launch."""
        with self.torch.cuda.device(self.device):
            rc = _fastpol_capi.lib.aquafast_refresh(self._src.data_ptr(), int(_policy_capi.lib.aquapol_weights_bytes()),
                                                    self._map.data_ptr(), self._blob.data_ptr(), self.networks, self._stream())
        self.last_error = "" if rc == 0 else _fastpol_capi.last_error()
        _fastpol_capi.check(rc, "aquafast_refresh")
        return self

    def load(self, layers):
        """source.load(layers) followed by refresh()"""
        self.source.load(layers)
        return self.refresh()

    # ------------------------------------------------------------------ the path
    def launch(self, in_ptr, ld, normalised, n, env_offset, epsilon, seed, tick, tick_base_ptr, action_ptr, q_ptr, q_ld,
               q_taken_ptr, stream):
        """aquafast_act_f16 on raw pointers, QNetwork.launch's signature -> return code.  BatchedAqua turns a non-zero code
        into an exception with the policy library's checker; this library's own message is kept in last_error."""
        eps = self.epsilon
        rc = _fastpol_capi.lib.aquafast_act_f16(self._blob.data_ptr(), self.networks, self.seg, in_ptr, ld, int(bool(normalised)), n,
                                                env_offset, float(epsilon), None if eps is None else eps.data_ptr(),
                                                int(seed) & ((1 << 64) - 1), int(tick) & ((1 << 64) - 1), tick_base_ptr, action_ptr,
                                                q_ptr, q_ld, q_taken_ptr, stream)
        self.last_error = "" if rc == 0 else _fastpol_capi.last_error()
        return rc

    def _reraise(self, e):
        if self.last_error:
            raise type(e)("aquafast_act_f16: %s" % self.last_error) from None
        raise e

    def act(self, env_or_buffer, epsilon=0.0, **kw):
        """QNetwork.act() on the fast path (for a bank: world i acts with network i // seg, and the bank's epsilon array,
        when set, replaces `epsilon` per network).  -> the action tensor [n]"""
        self.last_error = ""
        try:
            return QNetwork.act(self, env_or_buffer, epsilon, **kw)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)

    def q_values(self, buffer, n=None, out=None):
        """QNetwork.q_values() on the fast path -> float32 [3][n]"""
        self.last_error = ""
        try:
            return QNetwork.q_values(self, buffer, n, out)
        except (ValueError, _policy_capi.AquaPolicyError) as e:
            self._reraise(e)


def fast_blob_of(layers):
    """the fast blob of a layer stack on the host (numpy uint8): aquafast_pack_host of the packed float32 blob"""
    return _fastpol_capi.pack_host(_policy_capi.pack_weights(layers))

