"""Device-resident experience ring for a batch of worlds.

Reference being replaced: the DQN's experience buffer, main/impl/dqn.py:174 (`exp_buffer.append([state,
pred_action, reward, next_state, done])`, a Python deque of per-step lists) and its sampler, dqn.py:251-260
(`random.sample` + `np.vstack`).  Here one batched step appends one transition per world, struct-of-arrays,
straight from the environment's device buffers -- nothing crosses PCIe:

    s     float32 [5][capacity]   normalised observation before the step (main/impl/utils.py:15-33)
    a     uint8   [capacity]      discrete action          | float32 [2][capacity] continuous thrusts
    r     float32 [capacity]
    s2    float32 [5][capacity]   normalised observation after the step
    d     uint8   [capacity]      termination code (0 none, 1 collided, 2 time, 3 success); done = d != 0
    ok    uint8   [capacity]      1 for a real transition, 0 for a world that was restarting (next-step mode: that
                                  step reports reward 0 / term 0 and is not an experience)

The batch lands in consecutive slots (cursor .. cursor + N - 1, modulo capacity), so both sides of the copy are
coalesced; the copies are the C ABI's aqua_ring_write_* kernels on the environment's stream.

DeviceReplayRing is the same ring with cursor and size in device memory (libaqua_replay.so): one launch before the step,
one after it, and a minibatch draw that a captured graph replays correctly.
"""
import ctypes

from . import _capi


class ReplayRing(object):
    def __init__(self, env, capacity):
        torch = env.torch
        if env.obs_norm_buf is None:
            raise RuntimeError("ReplayRing stores the normalised observation: construct the env with normalized_obs=True")
        if capacity < env.num_envs:
            raise ValueError("capacity (%d) must hold at least one batched step (%d worlds)" % (capacity, env.num_envs))
        self.env = env
        self.capacity = int(capacity)
        dev = env.device
        c = self.capacity
        self.s = torch.zeros((5, c), dtype=torch.float32, device=dev)
        self.s2 = torch.zeros((5, c), dtype=torch.float32, device=dev)
        self.r = torch.zeros(c, dtype=torch.float32, device=dev)
        self.d = torch.zeros(c, dtype=torch.uint8, device=dev)
        self.ok = torch.zeros(c, dtype=torch.uint8, device=dev)
        self.a = torch.zeros((2, c), dtype=torch.float32, device=dev) if env.continuous else \
            torch.zeros(c, dtype=torch.uint8, device=dev)
        self._live = torch.zeros(env.ld, dtype=torch.uint8, device=dev)
        self.cursor = 0          # next slot
        self.size = 0            # filled slots (<= capacity)
        self._open = False

    # ------------------------------------------------------------------ writing
    def _f32(self, ring, src, src_ld, rows):
        e = self.env
        _capi.check(_capi.lib.aqua_ring_write_f32(ring.data_ptr(), self.capacity, self.capacity, self.cursor, src.data_ptr(),
                                                  src_ld, rows, e.num_envs, e._stream()), "aqua_ring_write_f32")

    def _u8(self, ring, src, src_ld, rows):
        e = self.env
        _capi.check(_capi.lib.aqua_ring_write_u8(ring.data_ptr(), self.capacity, self.capacity, self.cursor, src.data_ptr(),
                                                 src_ld, rows, e.num_envs, e._stream()), "aqua_ring_write_u8")

    def before_step(self, action):
        """Record (s, a) of the step about to be taken.  `action`: the tensor that will be passed to env.step()
        (uint8 [N] / float32 [2][ld] soa for continuous worlds)."""
        e = self.env
        torch = e.torch
        with torch.cuda.device(e.device):
            self._f32(self.s, e.obs_norm_buf, e.ld, 5)
            if e.continuous:
                if action.dim() != 2 or action.shape[0] != 2 or action.dtype != torch.float32 or action.stride(1) != 1:
                    raise ValueError("continuous actions are recorded from a float32 [2][>=N] tensor")
                self._f32(self.a, action, action.stride(0), 2)
            else:
                if action.dtype != torch.uint8 or action.dim() != 1 or action.numel() < e.num_envs:
                    raise ValueError("discrete actions are recorded from a uint8 [>=N] tensor")
                self._u8(self.a, action, action.numel(), 1)
            # worlds that are about to be restarted instead of stepped (next-step mode) are not experiences
            self._live.copy_((e.time >= 0) | (e.time <= -3))      # time markers: include/aqua_hip.h
            self._u8(self.ok, self._live, e.ld, 1)
        self._open = True

    def after_step(self, reward=None, term=None):
        """Record (r, s', d) of the step just taken into the same slots and advance the cursor."""
        if not self._open:
            raise RuntimeError("after_step() without before_step()")
        e = self.env
        reward = e.reward if reward is None else reward
        term = e.term if term is None else term
        with e.torch.cuda.device(e.device):
            self._f32(self.r, reward, reward.numel(), 1)
            self._f32(self.s2, e.obs_norm_buf, e.ld, 5)
            self._u8(self.d, term, term.numel(), 1)
        self.cursor = (self.cursor + e.num_envs) % self.capacity
        self.size = min(self.capacity, self.size + e.num_envs)
        self._open = False

    # ------------------------------------------------------------------ reading (dqn.py:251-260)
    def sample(self, batch_size, generator=None):
        """-> (s [B,5], a [B] | [B,2], r [B], s2 [B,5], done bool [B]) of uniformly drawn real transitions."""
        torch = self.env.torch
        if self.size == 0:
            raise RuntimeError("the ring is empty")
        idx = torch.randint(0, self.size, (int(batch_size) * 2,), device=self.env.device, generator=generator)
        idx = idx[self.ok[idx] != 0][:int(batch_size)]          # restarting worlds are < 2 % of the slots
        a = self.a[:, idx].t() if self.env.continuous else self.a[idx]
        return self.s[:, idx].t(), a, self.r[idx], self.s2[:, idx].t(), self.d[idx] != 0


class _LearnerView(object):
    """what DQNLearner.update(..., idx=...) reads of a DeviceReplayRing: the six tensors, capacity, and size = capacity"""

    def __init__(self, ring):
        self.s, self.a, self.r, self.s2, self.d, self.ok = ring.s, ring.a, ring.r, ring.s2, ring.d, ring.ok
        self.capacity = self.size = ring.capacity


class DeviceReplayRing(object):
    """ReplayRing with its cursor and size in DEVICE memory (libaqua_replay.so, include/aqua_replay.h): the same six rows,
    written by ONE launch before the step and ONE after it, and a minibatch draw that reads the size where it lives -- so
    append, draw and DQNLearner.update(view, B, idx=idx) replay correctly from a captured graph (trainer.DQNLoop).

        header  int64 [4]   cursor, size, first slot of the batch opened last, batches closed

    before_step(), after_step(), draw() and sample() do not allocate (given their `out`), synchronise or read back;
    filled(), position() and state_dict() are host reads.  There is no CPU path."""

    def __init__(self, env, capacity):
        torch = env.torch
        dev = torch.device(env.device)
        if dev.type != "cuda":
            raise RuntimeError("DeviceReplayRing runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (env.device,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: DeviceReplayRing has no CPU path")
        from . import _replay_capi                    # (lazily: ReplayRing does not depend on libaqua_replay.so)
        self._capi = _replay_capi
        if env.obs_norm_buf is None:
            raise RuntimeError("DeviceReplayRing stores the normalised observation: construct the env with normalized_obs=True")
        if capacity < env.num_envs:
            raise ValueError("capacity (%d) must hold at least one batched step (%d worlds)" % (capacity, env.num_envs))
        if capacity > _replay_capi.MAX_CAPACITY:
            raise ValueError("capacity (%d) above %d" % (capacity, _replay_capi.MAX_CAPACITY))
        self.torch, self.env, self.device = torch, env, dev
        self.capacity = int(capacity)
        c = self.capacity
        self.s = torch.zeros((5, c), dtype=torch.float32, device=dev)
        self.s2 = torch.zeros((5, c), dtype=torch.float32, device=dev)
        self.r = torch.zeros(c, dtype=torch.float32, device=dev)
        self.d = torch.zeros(c, dtype=torch.uint8, device=dev)
        self.ok = torch.zeros(c, dtype=torch.uint8, device=dev)
        self.a = torch.zeros((2, c), dtype=torch.float32, device=dev) if env.continuous else \
            torch.zeros(c, dtype=torch.uint8, device=dev)
        self.header = torch.zeros(_replay_capi.HEADER_WORDS, dtype=torch.int64, device=dev)
        self._draws = torch.zeros(1, dtype=torch.int64, device=dev)      # the counter that keys sample(B, <seed>)
        self._kind = _replay_capi.ACT_F32X2 if env.continuous else _replay_capi.ACT_U8
        self._open = False

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _action(self, action):
        """-> (pointer, action_ld) of the tensor that will be passed to env.step()"""
        e, torch = self.env, self.torch
        if not isinstance(action, torch.Tensor) or action.device != self.device:
            raise ValueError("actions are recorded from a tensor on %s" % (self.device,))
        if e.continuous:
            if action.dim() != 2 or action.shape[0] != 2 or action.dtype != torch.float32 or action.stride(1) != 1 \
                    or action.shape[1] < e.num_envs:
                raise ValueError("continuous actions are recorded from a float32 [2][>=N] tensor")
            return action.data_ptr(), action.stride(0)
        if action.dtype != torch.uint8 or action.dim() != 1 or action.numel() < e.num_envs or not action.is_contiguous():
            raise ValueError("discrete actions are recorded from a uint8 [>=N] tensor")
        return action.data_ptr(), action.numel()

    def _open_launch(self, action_ptr, action_ld, s):
        """aquarpl_open on raw pointers -> return code (callers that capture graphs check it themselves)"""
        e = self.env
        return self._capi.lib.aquarpl_open(self.header.data_ptr(), self.s.data_ptr(), self.a.data_ptr(), self.ok.data_ptr(),
                                           self.capacity, self.capacity, e.obs_norm_buf.data_ptr(), e.ld, action_ptr, self._kind,
                                           action_ld, e.time.data_ptr(), e.num_envs, s)

    def _close_launch(self, reward_ptr, term_ptr, s):
        e = self.env
        return self._capi.lib.aquarpl_close(self.header.data_ptr(), self.r.data_ptr(), self.s2.data_ptr(), self.d.data_ptr(),
                                            self.capacity, self.capacity, reward_ptr, e.obs_norm_buf.data_ptr(), e.ld, term_ptr,
                                            e.num_envs, s)

    def _vec(self, t, dtype, what):
        torch = self.torch
        n = self.env.num_envs
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or t.dim() != 1 or t.numel() < n \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s [>=%d] tensor on %s" % (what, dtype, n, self.device))
        return t.data_ptr()

    # ------------------------------------------------------------------ writing
    def before_step(self, action):
        """Record (s, a, ok) of the step about to be taken: one launch.  `action`: the tensor that will be passed to
        env.step() (uint8 [>=N] / float32 [2][>=N] soa for continuous worlds)."""
        ptr, ld = self._action(action)
        with self.torch.cuda.device(self.device):
            self._capi.check(self._open_launch(ptr, ld, self._stream()), "aquarpl_open")
        self._open = True

    def after_step(self, reward=None, term=None):
        """Record (r, s', d) of the step just taken into the same slots and advance the device cursor: one launch."""
        if not self._open:
            raise RuntimeError("after_step() without before_step()")
        e, torch = self.env, self.torch
        r_ptr = self._vec(e.reward if reward is None else reward, torch.float32, "reward")
        t_ptr = self._vec(e.term if term is None else term, torch.uint8, "term")
        with torch.cuda.device(self.device):
            self._capi.check(self._close_launch(r_ptr, t_ptr, self._stream()), "aquarpl_close")
        self._open = False

    # ------------------------------------------------------------------ reading
    def filled(self):
        """slots filled so far (a host read)"""
        return int(self.header[1])

    def position(self):
        """the next slot (a host read)"""
        return int(self.header[0])

    def learner_view(self):
        """the ring as DQNLearner.update(view, B, idx=ring.draw(B, learner)) reads it: size = capacity, because a slot
        never written has ok == 0 and the draw has already used the true size"""
        return _LearnerView(self)

    def _idx(self, batch_size, out):
        torch = self.torch
        B = int(batch_size)
        if B < 0 or B > self._capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [0, %d]" % (B, self._capi.MAX_BATCH))
        if out is None:
            out = torch.empty(max(B, 1), dtype=torch.int32, device=self.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != self.device or out.dim() != 1 \
                or out.numel() < B or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 [>=%d] tensor on %s" % (B, self.device))
        return B, out

    def _draw_launch(self, t_dev, seed, idx, B):
        with self.torch.cuda.device(self.device):
            self._capi.check(self._capi.lib.aquarpl_draw(self.header.data_ptr(), self.ok.data_ptr(), self.capacity, t_dev.data_ptr(),
                                                         int(seed) & ((1 << 64) - 1), idx.data_ptr(), B, self._stream()), "aquarpl_draw")

    def draw(self, batch_size, learner, out=None):
        """The slots `learner`'s NEXT update would draw by itself (DQNLearner.update(ring, B) with idx=None), from the device
        size: one launch -> int32 [B], -1 where four attempts met no real transition."""
        if learner.device != self.device:
            raise ValueError("the ring is on %s, the learner on %s" % (self.device, learner.device))
        B, out = self._idx(batch_size, out)
        self._draw_launch(learner.t, learner.seed, out, B)
        return out[:B]

    def sample(self, batch_size, learner_or_seed=0, out=None, idx=None):
        """A capturable ReplayRing.sample(): fixed shapes, two launches (draw, gather) -> (s [B,5], a [B] | [B,2], r [B],
        s2 [B,5], done uint8 [B], valid uint8 [B]); a sample that does not exist is a zero row with valid == 0.
        learner_or_seed: a DQNLearner (the slots of its next update) or an integer seed (draws keyed by the ring's own
        counter, which one small torch operation then advances).  out: the six tensors to fill; idx: int32 [>=B] scratch."""
        torch = self.torch
        B, idx = self._idx(batch_size, idx)
        if hasattr(learner_or_seed, "t") and hasattr(learner_or_seed, "seed"):
            if learner_or_seed.device != self.device:
                raise ValueError("the ring is on %s, the learner on %s" % (self.device, learner_or_seed.device))
            self._draw_launch(learner_or_seed.t, learner_or_seed.seed, idx, B)
        else:
            self._draw_launch(self._draws, int(learner_or_seed), idx, B)
            self._draws += 1
        return self.gather(idx, B, out)

    def gather(self, idx, batch_size=None, out=None):
        """the rows of the slots idx (int32) names: one launch -> the six tensors of sample()"""
        torch = self.torch
        B = int(idx.numel() if batch_size is None else batch_size)
        B, idx = self._idx(B, idx)
        cont = self.env.continuous
        shapes = (((B, 5), torch.float32), ((B, 2) if cont else (B,), torch.float32 if cont else torch.uint8), ((B,), torch.float32),
                  ((B, 5), torch.float32), ((B,), torch.uint8), ((B,), torch.uint8))
        if out is None:
            out = tuple(torch.empty(shape, dtype=dtype, device=self.device) for shape, dtype in shapes)
        if len(out) != 6:
            raise ValueError("out: the six tensors s, a, r, s2, done, valid")
        for t, (shape, dtype) in zip(out, shapes):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or tuple(t.shape) != shape \
                    or not t.is_contiguous():
                raise ValueError("out: expected a contiguous %s %s tensor on %s" % (dtype, shape, self.device))
        with torch.cuda.device(self.device):
            self._capi.check(self._capi.lib.aquarpl_gather(
                idx.data_ptr(), B, self.s.data_ptr(), self.a.data_ptr(), self.r.data_ptr(), self.s2.data_ptr(), self.d.data_ptr(),
                self.ok.data_ptr(), self.capacity, self.capacity, self._kind, *(t.data_ptr() for t in out), self._stream()),
                "aquarpl_gather")
        return tuple(out)

    # ------------------------------------------------------------------ resuming
    _STATE = ("s", "a", "r", "s2", "d", "ok", "header", "_draws")

    def state_dict(self):
        out = {name.lstrip("_"): getattr(self, name).detach().cpu().clone() for name in self._STATE}
        out["hyper"] = {"capacity": self.capacity, "continuous": bool(self.env.continuous), "open": self._open}
        return out

    def load_state_dict(self, state):
        """Resume bit for bit: the six rows and the header (cursor, size, the batch opened last, batches closed)."""
        torch = self.torch
        h = state.get("hyper", {})
        if h.get("capacity", self.capacity) != self.capacity or h.get("continuous", bool(self.env.continuous)) != bool(self.env.continuous):
            raise ValueError("the state was saved with capacity=%r continuous=%r" % (h.get("capacity"), h.get("continuous")))
        for name in self._STATE:
            dst, src = getattr(self, name), torch.as_tensor(state[name.lstrip("_")])
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name.lstrip("_"), dst.dtype, tuple(dst.shape)))
        for name in self._STATE:
            getattr(self, name).copy_(torch.as_tensor(state[name.lstrip("_")]))
        self._open = bool(h.get("open", False))
        return self
