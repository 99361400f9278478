"""SegmentTracker: the episode bookkeeping of ONE training of the reference -- epsilon = max(epsilon * decay, final) once per
finished episode (main/impl/dqn.py:139-141,184) and mean_last_100 of reward and success (dqn.py:196-198) -- kept for every
SEGMENT of a batch of worlds, on the device by libaqua_segments.so (include/aqua_segments.h).  Segment p is the worlds
[env_offset + p * seg, env_offset + (p + 1) * seg): those of network p of a QNetworkBank.

It accounts no step itself.  It consumes the records the EpisodeTracker's after_step() has just appended to its log, with a
device cursor of its own: one account() after every tracker.after_step(), which is what after_step() here does.  All state
is device memory -- counters per segment, the schedules (`epsilon`, float32 [P], ready to be bank.epsilon), a window of
the last W episodes per segment and its published mean return, mean length and success rate.  account() is one launch with
no allocation, no synchronisation and no host read: it works unchanged inside torch.cuda.graph and aqua_graph_begin/end.
Only counts() and state_dict() read back.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _segments_capi


def _per_segment(value, P, what):
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(P, float(a))
    if a.shape != (P,):
        raise ValueError("epsilon: %s must be a number or %d of them, got shape %s" % (what, P, a.shape))
    return a


class SegmentTracker(object):
    def __init__(self, tracker, seg, segments, window=100, epsilon=None):
        """tracker: the EpisodeTracker whose log is consumed.  seg: worlds per segment; segments: P of them (P * seg may
        exceed the batch: the last segment then holds fewer worlds; a world beyond P * seg belongs to none and its episodes
        are counted as stray).  window: W, the episodes the statistics look back on (the reference: 100).
        epsilon: (init, final, decay) of dqn.py's default_hyperparam, each a number or a sequence of P; decay >= 1 means
        "episodes to reach final" and is converted as dqn.py:139-140 does.  None: no schedule.
        Records already in the log are not consumed: the cursor starts at the tracker's."""
        if not all(hasattr(tracker, name) for name in ("log_world", "_counts", "capacity", "env", "torch", "device")):
            raise ValueError("expected an EpisodeTracker (it runs on an AMD GPU through HIP only; there is no CPU path)")
        torch = tracker.torch
        dev = tracker.device
        self.torch, self.tracker, self.device = torch, tracker, dev
        self.seg, self.segments, self.window = int(seg), int(segments), int(window)
        P, W = self.segments, self.window
        if not (1 <= self.seg <= _segments_capi.MAX_WORLDS):
            raise ValueError("seg=%d: must be in [1, %d]" % (self.seg, _segments_capi.MAX_WORLDS))
        if not (1 <= P <= _segments_capi.MAX_SEGMENTS):
            raise ValueError("segments=%d: must be in [1, %d]" % (P, _segments_capi.MAX_SEGMENTS))
        if not (1 <= W <= _segments_capi.MAX_WINDOW):
            raise ValueError("window=%d: must be in [1, %d]" % (W, _segments_capi.MAX_WINDOW))
        self.header = torch.zeros(_segments_capi.HEADER, dtype=torch.int64, device=dev)            # the library's uint64 [4]
        self._counts = torch.zeros((P, _segments_capi.COUNTS), dtype=torch.int64, device=dev)      # the library's uint64 [P][8]
        self.win_ret = torch.zeros((P, W), dtype=torch.float32, device=dev)
        self.win_len = torch.zeros((P, W), dtype=torch.int32, device=dev)
        self.win_code = torch.zeros((P, W), dtype=torch.uint8, device=dev)
        self.mean_return = torch.zeros(P, dtype=torch.float32, device=dev)
        self.mean_length = torch.zeros(P, dtype=torch.float32, device=dev)
        self.success_rate = torch.zeros(P, dtype=torch.float32, device=dev)
        self.eps_init = self.eps_final = self.decay = None
        self.hyper = self._eps_state = self.epsilon = None
        if epsilon is not None:
            init, final, decay = (_per_segment(v, P, what) for v, what in zip(epsilon, ("init", "final", "decay")))
            if not ((init >= 0.0).all() and (final >= 0.0).all() and (decay > 0.0).all()):
                raise ValueError("epsilon=(init, final, decay): init, final >= 0 and decay > 0, got %r" % (epsilon,))
            factor = np.empty(P, dtype=np.float64)
            for p in range(P):                                      # dqn.py:139-140, in Python floats as EpisodeTracker does it
                i, f, d = float(init[p]), float(final[p]), float(decay[p])
                factor[p] = d if d < 1 else ((f / i) ** (1 / d) if i > 0.0 else 1.0)
            if not ((factor > 0.0).all() and (factor <= 1.0).all()):
                raise ValueError("epsilon=%r: a decay factor is outside (0, 1]: %r" % (epsilon, factor))
            self.eps_init, self.eps_final, self.decay = init, final, factor
            self.hyper = torch.from_numpy(np.stack([factor, final], axis=1).copy()).to(dev)
            self._eps_state = torch.from_numpy(init.copy()).to(dev)
            self.epsilon = torch.from_numpy(init.astype(np.float32)).to(dev)
        self.header[0:1].copy_(tracker._counts[0:1])                # seen = the log cursor: a device copy, no host read

    # ------------------------------------------------------------------ the path
    def account(self):
        """The launch alone, on torch's current stream: account the records the tracker's last after_step() appended."""
        torch, t = self.torch, self.tracker
        sched = self._eps_state is not None
        with torch.cuda.device(self.device):
            rc = _segments_capi.lib.aquaseg_account(
                t.log_ret.data_ptr(), t.log_len.data_ptr(), t.log_code.data_ptr(), t.log_world.data_ptr(), t.capacity,
                t._counts.data_ptr(), int(t.env.env_offset), t.num_envs, self.seg, self.segments, self.window,
                self.header.data_ptr(), self._counts.data_ptr(), self.hyper.data_ptr() if sched else None,
                self._eps_state.data_ptr() if sched else None, self.epsilon.data_ptr() if sched else None,
                self.win_ret.data_ptr(), self.win_len.data_ptr(), self.win_code.data_ptr(),
                self.mean_return.data_ptr(), self.mean_length.data_ptr(), self.success_rate.data_ptr(),
                ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _segments_capi.check(rc, "aquaseg_account")

    def after_step(self, reward=None, term=None, time=None):
        """tracker.after_step(reward, term, time) followed by account(): three launches"""
        self.tracker.after_step(reward, term, time)
        self.account()

    # ------------------------------------------------------------------ reading (a host read)
    def counts(self):
        """-> {"segments": [{"episodes", "collided", "timeout", "success", "steps"} per segment], "missed", "stray"}: steps are
        those of the segment's finished episodes; missed counts the calls that found more new records than one step can
        append (account() calls were skipped; those records are lost to the statistics); stray the records of worlds that
        belong to no segment"""
        h = [int(v) for v in self.header.cpu().numpy().view(np.uint64)]
        c = self._counts.cpu().numpy().view(np.uint64)
        rows = [{"episodes": int(r[0]), "collided": int(r[1]), "timeout": int(r[2]), "success": int(r[3]), "steps": int(r[4])} for r in c]
        return {"segments": rows, "missed": h[1], "stray": h[2]}

    # ------------------------------------------------------------------ resuming
    _STATE = ("header", "_counts", "win_ret", "win_len", "win_code", "mean_return", "mean_length", "success_rate",
              "hyper", "_eps_state", "epsilon")

    def state_dict(self):
        out = {}
        for name in self._STATE:
            t = getattr(self, name)
            out[name.lstrip("_")] = None if t is None else t.detach().cpu().clone()
        out["shape"] = {"seg": self.seg, "segments": self.segments, "window": self.window}
        return out

    def load_state_dict(self, state):
        """Resume bit for bit: the cursor, the counters, the windows, the statistics, the schedules and their parameters.
        The cursor is the saved one: load the tracker's state along with this."""
        torch = self.torch
        shape = state.get("shape", {})
        for key in ("seg", "segments", "window"):
            if shape.get(key, getattr(self, key)) != getattr(self, key):
                raise ValueError("the state was saved with %s=%r" % (key, shape.get(key)))
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
        if self.hyper is not None:
            h = self.hyper.cpu().numpy()
            self.decay, self.eps_final = h[:, 0].copy(), h[:, 1].copy()
        return self

    def reset_stats(self):
        """Forget the statistics: counters, windows, published means, missed and stray; the schedules are back at their
        initial values and the cursor at the tracker's (call it after tracker.reset_stats(), not before)."""
        for name in self._STATE[:-3]:
            getattr(self, name).zero_()
        self.header[0:1].copy_(self.tracker._counts[0:1])
        if self._eps_state is not None:
            self._eps_state.copy_(self.torch.from_numpy(self.eps_init.copy()))
            self.epsilon.copy_(self.torch.from_numpy(self.eps_init.astype(np.float32)))
