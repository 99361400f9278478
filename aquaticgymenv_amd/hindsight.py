"""Hindsight experience replay on the device: the goals of a minibatch draw relabelled from the experience ring
(libaqua_her.so, csrc/aqua_her.h; Andrychowicz et al., 2017, strategy "future").

The observation is (x, y, theta, gx, gy), and whenever a step ends in neither a collision nor the time limit its reward and
termination depend on (previous position, new position, goal) alone (gym_aqua/envs/aqua.py:206-211, 392-395, 421-422).  A
stored transition with d == 0 is therefore replayed EXACTLY under another goal: two columns are overwritten and one reward is
recomputed.  HindsightReplay does that for every sample of a draw, in ONE launch, with a share `ratio` of the eligible samples
given a goal their own world reached within the next `horizon` steps of the same episode.  The learners are then called
unchanged, on the staged rows:

    idx = ring.draw(B, learner, out=idx)
    her.relabel(idx, learner)
    learner.update(her.view, B, idx=her.idx)

    learners.draw(ring, B, out=idx)
    her.relabel(idx, learners)
    learners.update(her.view, B, her.idx)

The relabelling draws are Philox draws keyed like the minibatch draw of the same update -- the learner's seed and update
counter, or those of every network of a bank, read where they live -- on a stream of their own: a captured graph relabels
afresh at every replay, and eager and replayed runs hold the same bits.  With ratio = 0 the staged rows are the ring's rows of
the drawn slots bit for bit.  Nothing is kept between calls.  There is no CPU path.
"""
import ctypes

from .nstep import _StagedView


class HindsightReplay(object):
    def __init__(self, ring, batch_size, networks=1, horizon=32, ratio=0.8):
        """ring: a DeviceReplayRing whose capacity is a multiple of its env's num_envs; batch_size: samples per network and
        call; networks: P, the rows of the draw (1 for a DQNLearner, the bank's number of networks for a DQNLearnerBank);
        horizon: H, how many steps ahead a goal may lie, 1 .. MAX_HORIZON; ratio: the share of the eligible samples to
        relabel, in [0, 1].  Anything else is a ValueError.  Owns the staged rows (s, s2 float32 [5][P B]; r float32; a
        uint8, or float32 [2][P B] for continuous worlds; d, ok uint8), k and m (uint8 [P B]: k + 1 of a relabelled sample,
        else 0, and the number M of candidate steps), idx int32 [P][B] = p B + j (the constant draw that names every staged
        sample) and view, the staged rows as the learners read a ring."""
        if getattr(ring, "header", None) is None or not hasattr(ring, "env"):
            raise ValueError("expected a DeviceReplayRing")
        torch = ring.torch
        if ring.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("HindsightReplay runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (ring.device,))
        from . import _her_capi                       # (lazily: nothing else depends on libaqua_her.so)
        self._capi = _her_capi
        B, P, H = int(batch_size), int(networks), int(horizon)
        if not 1 <= B <= _her_capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [1, %d]" % (B, _her_capi.MAX_BATCH))
        if not 1 <= P <= _her_capi.MAX_NETWORKS:
            raise ValueError("networks=%d: must be in [1, %d]" % (P, _her_capi.MAX_NETWORKS))
        if not 1 <= H <= _her_capi.MAX_HORIZON:
            raise ValueError("horizon=%d: must be in [1, %d]" % (H, _her_capi.MAX_HORIZON))
        try:
            self.threshold = _her_capi.threshold(ratio)
        except (TypeError, ValueError):
            raise ValueError("ratio=%r: must be a number in [0, 1]" % (ratio,))
        if ring.capacity % ring.env.num_envs != 0:
            raise ValueError("the ring's capacity (%d) must be a multiple of the batch (%d worlds): the next step of a world is then "
                             "the slot one batch further" % (ring.capacity, ring.env.num_envs))
        self.torch, self.ring, self.device = torch, ring, ring.device
        self.batch_size, self.networks, self.samples, self.horizon, self.ratio = B, P, P * B, H, float(ratio)
        self.idx = torch.arange(P * B, dtype=torch.int32, device=self.device).reshape(P, B)
        self._rows = self._staging()
        self.s, self.a, self.r, self.s2, self.d, self.ok, self.k, self.m = self._rows
        self.view = _StagedView(self._rows[:6], P * B)

    # ------------------------------------------------------------------ plumbing
    def _staging(self):
        """-> (s, a, r, s2, d, ok, k, m), zeroed, with the pitch P * B"""
        torch, dev, m = self.torch, self.device, self.samples
        a = torch.zeros((2, m), dtype=torch.float32, device=dev) if self.ring.env.continuous else torch.zeros(m, dtype=torch.uint8, device=dev)
        u8 = lambda: torch.zeros(m, dtype=torch.uint8, device=dev)      # noqa: E731
        return (torch.zeros((5, m), dtype=torch.float32, device=dev), a, torch.zeros(m, dtype=torch.float32, device=dev),
                torch.zeros((5, m), dtype=torch.float32, device=dev), u8(), u8(), u8(), u8())

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _keys(self, source):
        """-> (t, seed, seed_dev) of a DQNLearner (a host seed) or a DQNLearnerBank (its device keys)"""
        torch, P = self.torch, self.networks
        t, keys = getattr(source, "t", None), getattr(source, "seed_dev", None)
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.device != self.device or tuple(t.shape) != (P,) \
                or not t.is_contiguous():
            raise ValueError("learner: expected a DQNLearner%s on %s whose update counter t is int64 [%d]"
                             % (" or a DQNLearnerBank" if P > 1 else "", self.device, P))
        if keys is not None:
            if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.device != self.device \
                    or tuple(keys.shape) != (P,) or not keys.is_contiguous():
                raise ValueError("learner: seed_dev must be a contiguous int64 [%d] tensor on %s" % (P, self.device))
            return t, self._capi.NO_SEED, keys
        if P != 1 or not hasattr(source, "seed"):
            raise ValueError("learner: %d networks need a DQNLearnerBank (its device keys seed_dev)" % P)
        return t, int(source.seed) & ((1 << 64) - 1), None

    def _launch(self, idx, t, seed, keys, rows):
        """aquaher_relabel on the ring: idx int32 [P][B]; t the update counters; seed a host integer or keys a device row;
        rows: the eight staged tensors"""
        ring, capi = self.ring, self._capi
        s, a, r, s2, d, ok, k, m = rows
        with self.torch.cuda.device(self.device):
            rc = capi.lib.aquaher_relabel(
                ring.header.data_ptr(), ring.s.data_ptr(), ring.a.data_ptr(), ring.r.data_ptr(), ring.s2.data_ptr(), ring.d.data_ptr(),
                ring.ok.data_ptr(), ring.capacity, ring.capacity, ring._kind, ring.env.num_envs,
                idx.data_ptr(), self.networks, self.batch_size, self.horizon, self.ratio, t.data_ptr(), seed,
                None if keys is None else keys.data_ptr(),
                s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(), ok.data_ptr(), self.samples,
                k.data_ptr(), m.data_ptr(), self._stream())
        capi.check(rc, "aquaher_relabel")

    # ------------------------------------------------------------------ the path
    def relabel(self, idx, learner):
        """Queue the relabelling of the draw `idx` (int32 [P][B], or [B] for one network: slots of the ring, -1 for none) on
        torch's current stream: one launch, no allocation, no host read.  learner: the DQNLearner, or the DQNLearnerBank of P
        networks, whose next update the draw is for: its counter t and its key(s) key the relabelling draws.  -> self.view"""
        torch, P, B = self.torch, self.networks, self.batch_size
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous() \
                or tuple(idx.shape) not in (((P, B),) if P > 1 else ((P, B), (B,))):
            raise ValueError("idx must be a contiguous int32 [%d][%d] tensor on %s" % (P, B, self.device))
        t, seed, keys = self._keys(learner)
        self._launch(idx, t, seed, keys, self._rows)
        return self.view

    def _warm_up(self, with_table=False):
        """the kernel once (the instance that reads a bank's keys with with_table), on scratch rows and a draw of -1, which
        names no sample: the staged rows keep their bytes"""
        torch = self.torch
        t = torch.zeros(self.networks, dtype=torch.int64, device=self.device)
        self._launch(torch.full_like(self.idx, -1), t, self._capi.NO_SEED, t if with_table else None, self._staging())
