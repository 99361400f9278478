"""EpisodeTracker: the episode bookkeeping of the reference's loops -- episode_reward, episode_steps, reward_list,
success_list and epsilon = max(epsilon * decay, final) once per finished episode (main/impl/dqn.py:139-141,151-200); Reward and
Success of one episode per run (Policy.test, main/testing/__init__.py:17-36, and TestPlotter.run_tests) -- for a batch of
worlds, on the device by libaqua_episodes.so (include/aqua_episodes.h).

All state is device memory: running return and length per world, a ring log of finished episodes in a deterministic order
(the worlds ending in one step are logged by ascending index), counters by termination code, and the epsilon schedule, whose
float32 copy `epsilon` the exploration pass reads on the device.  after_step() is two launches and explore() one, with no
allocation, no synchronisation and no host read: both work unchanged inside torch.cuda.graph and aqua_graph_begin/end.
Only counts(), last() and state_dict() read back.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _episodes_capi

CODES = {1: "collided", 2: "timeout", 3: "success"}          # termination codes of include/aqua_hip.h


class EpisodeTracker(object):
    def __init__(self, env, capacity=None, once=False, epsilon=None):
        """env: a BatchedAqua (or anything with its torch, device, num_envs, env_offset, reward, term, time attributes).
        capacity: records the log ring holds, default max(N, 65536), at least N.
        once: one episode per world (Policy.test / run_tests on an auto_reset=False batch): a world that has logged its
              episode is ignored from then on.
        epsilon: (init, final, decay) of dqn.py's default_hyperparam; decay >= 1 means "episodes to reach final" and is
              converted as dqn.py:139-140 does.  None: no schedule."""
        torch = env.torch
        dev = torch.device(env.device)
        if dev.type != "cuda":
            raise RuntimeError("EpisodeTracker runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (env.device,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: EpisodeTracker has no CPU path")
        self.torch, self.env, self.device = torch, env, dev
        n = int(env.num_envs)
        self.num_envs = n
        self.capacity = max(n, 65536) if capacity is None else int(capacity)
        if self.capacity < n:
            raise ValueError("capacity (%d) must hold at least one batched step (%d worlds)" % (self.capacity, n))
        self.once = bool(once)
        c = max(self.capacity, 1)
        self.ret = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        self.len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.finished = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) if self.once else None
        self.log_ret = torch.zeros(c, dtype=torch.float32, device=dev)
        self.log_len = torch.zeros(c, dtype=torch.int32, device=dev)
        self.log_code = torch.zeros(c, dtype=torch.uint8, device=dev)
        self.log_world = torch.zeros(c, dtype=torch.int64, device=dev)
        self._counts = torch.zeros(_episodes_capi.COUNTS, dtype=torch.int64, device=dev)       # the library's uint64 [8]
        self.eps_init = self.eps_final = self.decay = None
        self._eps_state = self.epsilon = None
        if epsilon is not None:
            init, final, decay = (float(v) for v in epsilon)
            if not (init >= 0.0 and final >= 0.0 and decay > 0.0):
                raise ValueError("epsilon=(init, final, decay): init, final >= 0 and decay > 0, got %r" % (epsilon,))
            if decay >= 1:                                      # dqn.py:139-140
                decay = (final / init) ** (1 / decay) if init > 0.0 else 1.0
            if not (0.0 < decay <= 1.0):
                raise ValueError("epsilon=%r: the decay factor %r is outside (0, 1]" % (epsilon, decay))
            self.eps_init, self.eps_final, self.decay = init, final, decay
            self._eps_state = torch.full((1,), init, dtype=torch.float64, device=dev)
            self.epsilon = torch.full((1,), init, dtype=torch.float32, device=dev)
        need = int(_episodes_capi.lib.aquaep_workspace_bytes(n))
        if need == 0:
            raise ValueError("num_envs=%d: must be in [0, %d]" % (n, _episodes_capi.MAX_WORLDS))
        self._workspace = torch.zeros(need, dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _vec(self, t, dtype, what):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or t.dim() != 1 \
                or t.numel() < self.num_envs or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s [>=%d] tensor on %s" % (what, dtype, self.num_envs, self.device))
        return t.data_ptr()

    # ------------------------------------------------------------------ the path
    def after_step(self, reward=None, term=None, time=None):
        """Account the batched step just taken, on torch's current stream.  reward float32 [>=N], term uint8 [>=N], time
        int32 [>=N]: default the env's own buffers (an env without a time row: every world counts)."""
        torch, e = self.torch, self.env
        reward = e.reward if reward is None else reward
        term = e.term if term is None else term
        time = getattr(e, "time", None) if time is None else time
        r_ptr = self._vec(reward, torch.float32, "reward")
        t_ptr = self._vec(term, torch.uint8, "term")
        time_ptr = None if time is None else self._vec(time, torch.int32, "time")
        sched = self._eps_state is not None
        with torch.cuda.device(self.device):
            rc = _episodes_capi.lib.aquaep_after_step_f32(
                r_ptr, t_ptr, time_ptr, int(e.env_offset), self.num_envs,
                self.ret.data_ptr(), self.len.data_ptr(), self.finished.data_ptr() if self.once else None,
                self.log_ret.data_ptr(), self.log_len.data_ptr(), self.log_code.data_ptr(), self.log_world.data_ptr(), self.capacity,
                self._counts.data_ptr(), self._eps_state.data_ptr() if sched else None, self.epsilon.data_ptr() if sched else None,
                self.decay if sched else 1.0, self.eps_final if sched else 0.0,
                self._workspace.data_ptr(), self._workspace.numel(), self._stream())
        _episodes_capi.check(rc, "aquaep_after_step_f32")

    def explore(self, action, seed=None, tick=None, tick_base=None, epsilon=None):
        """Overwrite greedy actions (uint8 [>=N], in place) with the policy kernel's exploring draw wherever its uniform is
        below the DEVICE epsilon: qnet.act(env, epsilon=0, out=a); tracker.explore(a) equals qnet.act(env, epsilon=e, out=a)
        on the same tick bit for bit.  seed, tick, tick_base default to what QNetwork.act(env) uses for this env.  A q_taken
        written by the greedy call is stale for the explored worlds.  epsilon: a float32 [1] device tensor instead of the
        schedule's.  -> action[:N]"""
        torch, e = self.torch, self.env
        if getattr(e, "continuous", False):
            raise ValueError("the exploration pass (main/impl/dqn.py:212-228) is defined for discrete actions")
        eps = self.epsilon if epsilon is None else epsilon
        if eps is None:
            raise RuntimeError("explore(): construct the tracker with epsilon=(init, final, decay) or pass a device epsilon")
        if not isinstance(eps, torch.Tensor) or eps.dtype != torch.float32 or eps.device != self.device or eps.numel() < 1:
            raise ValueError("epsilon must be a float32 tensor on %s" % (self.device,))
        a_ptr = self._vec(action, torch.uint8, "action")
        tb_ptr = None
        if tick_base is not None:
            if not isinstance(tick_base, torch.Tensor) or tick_base.dtype != torch.int64 or tick_base.device != self.device \
                    or tick_base.numel() < 1:
                raise ValueError("tick_base must be an int64 tensor on %s" % (self.device,))
            tb_ptr = tick_base.data_ptr()
        seed = e.seed if seed is None else seed
        tick = e._tick if tick is None else tick
        with torch.cuda.device(self.device):
            rc = _episodes_capi.lib.aquaep_explore_u8(a_ptr, self.num_envs, int(e.env_offset), eps.data_ptr(),
                                                      int(seed) & ((1 << 64) - 1), int(tick) & ((1 << 64) - 1), tb_ptr, self._stream())
        _episodes_capi.check(rc, "aquaep_explore_u8")
        return action[:self.num_envs]

    # ------------------------------------------------------------------ reading (host reads)
    def counts(self):
        """-> {"episodes", "collided", "timeout", "success", "steps"}: episodes logged so far, by termination code, and the
        world-steps counted"""
        c = [int(v) for v in self._counts.cpu().numpy().view(np.uint64)]
        return {"episodes": c[0], "collided": c[1], "timeout": c[2], "success": c[3], "steps": c[4]}

    def last(self, k):
        """The newest min(k, logged, capacity) records, oldest first -> {"ret", "len", "code", "world"} of numpy arrays"""
        torch = self.torch
        logged = int(self._counts[0])
        m = max(0, min(int(k), logged, self.capacity))
        idx = (torch.arange(logged - m, logged, dtype=torch.int64, device=self.device) % max(self.capacity, 1))
        return {"ret": self.log_ret[idx].cpu().numpy(), "len": self.log_len[idx].cpu().numpy(),
                "code": self.log_code[idx].cpu().numpy(), "world": self.log_world[idx].cpu().numpy()}

    # ------------------------------------------------------------------ resuming
    _STATE = ("ret", "len", "finished", "log_ret", "log_len", "log_code", "log_world", "_counts", "_eps_state", "epsilon")

    def state_dict(self):
        out = {}
        for name in self._STATE:
            t = getattr(self, name)
            out[name.lstrip("_")] = None if t is None else t.detach().cpu().clone()
        out["hyper"] = {"capacity": self.capacity, "once": self.once, "eps_init": self.eps_init, "eps_final": self.eps_final,
                        "decay": self.decay}
        return out

    def load_state_dict(self, state):
        """Resume bit for bit: running returns and lengths, the log and its cursor, the counters, the schedule."""
        torch = self.torch
        h = state.get("hyper", {})
        if h.get("capacity", self.capacity) != self.capacity or h.get("once", self.once) != self.once:
            raise ValueError("the state was saved with capacity=%r once=%r" % (h.get("capacity"), h.get("once")))
        for name in self._STATE:
            dst, src = getattr(self, name), state[name.lstrip("_")]
            if (dst is None) != (src is None):
                raise ValueError("state[%r]: this tracker %s it" % (name.lstrip("_"), "lacks" if dst is None else "needs"))
            if dst is None:
                continue
            src = torch.as_tensor(src)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name.lstrip("_"), dst.dtype, tuple(dst.shape)))
            dst.copy_(src)
        if self._eps_state is not None:
            for key in ("eps_init", "eps_final", "decay"):
                if h.get(key) is not None:
                    setattr(self, key, float(h[key]))
        return self

    def reset_stats(self):
        """Forget everything: running returns and lengths, the log, the counters; the schedule is back at its initial value."""
        for name in self._STATE[:-2]:
            t = getattr(self, name)
            if t is not None:
                t.zero_()
        if self._eps_state is not None:
            self._eps_state.fill_(self.eps_init)
            self.epsilon.fill_(self.eps_init)


def evaluate(env, policy, max_steps=1001, poll=64):
    """The batched Policy.test / TestPlotter.run_tests (main/testing/__init__.py:17-36): one episode per world from the
    env's current state (call env.reset() first) under env.step(policy=policy), on an auto_reset=False batch.  Steps until
    every world has logged its episode -- the counter is read every `poll` steps -- or max_steps are taken.
    -> {"Reward" float32, "Success" bool, "Steps" int32, "Code" uint8}, numpy arrays indexed by world; a world that has
    not finished has Code 0 and its running return and length."""
    if int(env.auto_reset) != 0:
        raise ValueError("evaluate(): one episode per world needs an auto_reset=False batch")
    n = env.num_envs
    tracker = EpisodeTracker(env, capacity=n, once=True)
    poll = max(int(poll), 1)
    for step in range(int(max_steps)):
        env.step(policy=policy)
        tracker.after_step()
        if step % poll == poll - 1 and tracker.counts()["episodes"] == n:
            break
    rec = tracker.last(n)
    reward = tracker.ret[:n].cpu().numpy().copy()
    steps = tracker.len[:n].cpu().numpy().copy()
    code = np.zeros(n, dtype=np.uint8)
    w = rec["world"] - env.env_offset
    reward[w], steps[w], code[w] = rec["ret"], rec["len"], rec["code"]
    return {"Reward": reward, "Success": code == 3, "Steps": steps, "Code": code}
