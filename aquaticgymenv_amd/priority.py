"""Prioritised experience replay on the device (libaqua_prio.so, csrc/aqua_prio.h): the proportional variant of Schaul et
al. for every network of a DQNLearnerBank, over the one DeviceReplayRing of the batch.

Every network has a sum tree of fan-out 64 over its own slots of the ring; priorities are 20-bit fixed point integers, so
every partial sum is exact and the draw is reproducible bit for bit.  The uniform stages of a training iteration are replaced
one for one:

    ring.after_step();  per.insert()              # the batch just closed enters with the largest priority seen so far
    per.draw(B)                                   # instead of learners.draw(ring, B): slots by descent, importance weights
    per.update(view, B, per.idx)                  # instead of learners.update(...): the weights multiply the TD errors
    per.set()                                     # the drawn slots get the priorities of their new TD errors

Nothing here allocates (after the first draw of a batch size), synchronises or reads back: the four calls are seven launches
that capture into a HIP graph.  beta anneals from beta0 to 1 over `anneal` updates of the network, read from the learner
bank's device counters: a replayed graph anneals without being captured again.  With NStepReturns (nstep.py), fold per.idx
and pass the staged rows: per.update(nstep.view, B, nstep.idx, hyper=nstep.hyper); a window the fold dropped keeps its
priority.  A bank of one network covers a single training.  There is no CPU path.
"""
import ctypes

import numpy as np


class PrioritizedReplay(object):
    def __init__(self, ring, learners, alpha=0.6, beta0=0.4, anneal=100000, eps=1e-3):
        """ring: a DeviceReplayRing whose capacity is a multiple of its env's num_envs; learners: the DQNLearnerBank whose
        networks draw from it.  alpha, beta0 in [0, 1]; anneal >= 1 updates; eps > 0.  Owns tree (uint8, the P sum trees as
        aquaprio_layout lays them out), pmax uint32-in-int32 [P], and per batch size idx int32 [P][B], weight float32 [P][B],
        td float32 [P][B].  Anything else is a ValueError; no GPU is a RuntimeError."""
        if getattr(ring, "header", None) is None or not hasattr(ring, "env"):
            raise ValueError("expected a DeviceReplayRing")
        if not hasattr(learners, "networks") or not hasattr(learners, "seed_dev") or not hasattr(learners, "hyper"):
            raise ValueError("expected a DQNLearnerBank")
        torch = ring.torch
        if ring.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("PrioritizedReplay runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (ring.device,))
        if learners.device != ring.device:
            raise ValueError("the ring is on %s, the learner bank on %s" % (ring.device, learners.device))
        from . import _prio_capi                      # (lazily: nothing else depends on libaqua_prio.so)
        self._capi = _prio_capi
        N = int(ring.env.num_envs)
        if ring.capacity % N != 0:
            raise ValueError("the ring's capacity (%d) must be a multiple of the batch (%d worlds): a slot then belongs to one world, "
                             "and so to one network" % (ring.capacity, N))
        alpha, beta0, anneal, eps = float(alpha), float(beta0), int(anneal), float(eps)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("alpha=%r: must be in [0, 1]" % (alpha,))
        if not 0.0 <= beta0 <= 1.0:
            raise ValueError("beta0=%r: must be in [0, 1]" % (beta0,))
        if anneal < 1:
            raise ValueError("anneal=%r: must be >= 1" % (anneal,))
        if not 1e-300 <= eps <= 1e300:
            raise ValueError("eps=%r: must be positive" % (eps,))
        self.torch, self.ring, self.learners, self.device = torch, ring, learners, ring.device
        self.alpha, self.beta0, self.anneal, self.eps = alpha, beta0, anneal, eps
        self.networks = int(learners.networks)
        # a segment beyond the batch owns the whole batch: the same slots as a segment of N worlds
        self._shape = (int(ring.capacity), N, min(int(learners.seg), N), self.networks)
        self.layout = _prio_capi.layout(*self._shape)
        self.tree = self._tree()
        self.pmax = self._pmax()
        self.batch_size = 0
        self.idx = self.weight = self.td = self._q = None

    # ------------------------------------------------------------------ plumbing
    def _tree(self):
        """a zeroed tree buffer (torch's allocations are 512-byte aligned)"""
        t = self.torch.zeros(self.layout["bytes"], dtype=self.torch.uint8, device=self.device)
        if t.data_ptr() % 512 != 0:
            raise RuntimeError("the allocator returned a buffer that is not 512-byte aligned")
        return t

    def _pmax(self):
        return self.torch.full((self.networks,), self._capi.ONE, dtype=self.torch.int32, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _grow(self, batch_size):
        """idx, weight, td and the descent's scratch for this batch size (outside of a capture)"""
        B = int(batch_size)
        if not 1 <= B <= self._capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [1, %d]" % (B, self._capi.MAX_BATCH))
        if B != self.batch_size:
            torch, dev, P = self.torch, self.device, self.networks
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the buffers of a batch size are made outside of a graph capture: run one draw of this size first")
            self.idx = torch.full((P, B), -1, dtype=torch.int32, device=dev)
            self.weight = torch.zeros((P, B), dtype=torch.float32, device=dev)
            self.td = torch.full((P, B), -1.0, dtype=torch.float32, device=dev)
            self._q = torch.zeros((P, B), dtype=torch.int32, device=dev)
            self.batch_size = B
        self.learners._grow(B)
        return B

    def _rows(self, t, dtype, what):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or tuple(t.shape) != (self.networks, self.batch_size) \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s [%d][%d] tensor on %s" % (what, dtype, self.networks, self.batch_size, self.device))
        return t

    def _insert(self, tree, pmax, header):
        capi, ring = self._capi, self.ring
        with self.torch.cuda.device(self.device):
            rc = capi.lib.aquaprio_insert(tree.data_ptr(), tree.numel(), pmax.data_ptr(), *self._shape, header.data_ptr(),
                                          ring.ok.data_ptr(), self._stream())
        capi.check(rc, "aquaprio_insert")

    def _draw(self, tree, idx, weight, q):
        capi, lb = self._capi, self.learners
        with self.torch.cuda.device(self.device):
            rc = capi.lib.aquaprio_draw(tree.data_ptr(), tree.numel(), *self._shape, self.ring.header.data_ptr(), lb.t.data_ptr(),
                                        lb.seed_dev.data_ptr(), idx.data_ptr(), weight.data_ptr(), q.data_ptr(), self.batch_size,
                                        self.beta0, self.anneal, self._stream())
        capi.check(rc, "aquaprio_draw")

    def _set(self, tree, pmax, idx, td):
        capi = self._capi
        with self.torch.cuda.device(self.device):
            rc = capi.lib.aquaprio_set(tree.data_ptr(), tree.numel(), pmax.data_ptr(), *self._shape, idx.data_ptr(), td.data_ptr(),
                                       self.batch_size, self.alpha, self.eps, self._stream())
        capi.check(rc, "aquaprio_set")

    # ------------------------------------------------------------------ the path
    def insert(self):
        """Queue behind ring.after_step(): the batch just closed enters the trees, a real transition with its network's
        largest priority so far, anything else with 0.  One launch."""
        self._insert(self.tree, self.pmax, self.ring.header)

    def draw(self, batch_size=64, out=None):
        """The minibatch of every network's NEXT update by descent of its tree, and the importance weights that go with it:
        two launches -> idx int32 [P][B] (self.idx, or `out`), -1 where the network has no experience; self.weight [P][B]."""
        self._grow(batch_size)
        idx = self.idx if out is None else self._rows(out, self.torch.int32, "out")
        self._draw(self.tree, idx, self.weight, self._q)
        return idx

    def update(self, view, batch_size, idx, hyper=None):
        """DQNLearnerBank.update(view, batch_size, idx, hyper=hyper) with self.weight multiplied into the TD errors; the
        plain TD error of every sample goes to self.td (-1 for what is no sample).  Two launches -> learners.loss"""
        from . import _learner_capi
        torch, lb, capi = self.torch, self.learners, self._capi
        B = int(batch_size)
        if B != self.batch_size:
            raise ValueError("batch_size=%d: the weights are those of a draw of %d" % (B, self.batch_size))
        if view.a.dtype != torch.uint8 or view.a.dim() != 1:
            raise ValueError("the Q-network (main/impl/dqn.py) is defined for discrete actions: the ring holds continuous ones")
        if view.s.device != self.device:
            raise ValueError("the ring is on %s, the learner bank on %s" % (view.s.device, self.device))
        cap = int(view.capacity)
        for name, rows, dtype in (("s", 5, torch.float32), ("s2", 5, torch.float32), ("r", 1, torch.float32), ("a", 1, torch.uint8),
                                  ("d", 1, torch.uint8), ("ok", 1, torch.uint8)):
            t = getattr(view, name)
            if t.dtype != dtype or not t.is_contiguous() or t.numel() != rows * cap:
                raise ValueError("ring.%s must be a contiguous %s tensor of %d x %d" % (name, dtype, rows, cap))
        self._rows(idx, torch.int32, "idx")
        if hyper is None:
            hyper = lb.hyper
        elif not isinstance(hyper, torch.Tensor) or hyper.dtype != lb.hyper.dtype or hyper.device != self.device \
                or hyper.shape != lb.hyper.shape or not hyper.is_contiguous():
            raise ValueError("hyper must be a contiguous %s %s tensor on %s" % (lb.hyper.dtype, tuple(lb.hyper.shape), self.device))
        need = lb._grow(B)
        with torch.cuda.device(self.device):
            rc = capi.lib.aquaprio_update_f32(
                lb.theta.data_ptr(), lb.theta_target.data_ptr(), lb.m.data_ptr(), lb.v.data_ptr(), lb.t.data_ptr(), self.networks,
                view.s.data_ptr(), view.a.data_ptr(), view.r.data_ptr(), view.s2.data_ptr(), view.d.data_ptr(), view.ok.data_ptr(),
                cap, int(view.size), idx.data_ptr(), B,
                _learner_capi.STRATEGIES[lb.strategy] | _learner_capi.LOSSES[lb.loss_form], hyper.data_ptr(),
                lb.bank.tensor.data_ptr(), lb.target_tensor.data_ptr(), lb.perm.data_ptr(), lb.blob_floats,
                lb._workspace.data_ptr(), need, None, lb.grad.data_ptr(), lb.loss.data_ptr(),
                self.weight.data_ptr(), self.td.data_ptr(), self._stream())
        capi.check(rc, "aquaprio_update_f32")
        return lb.loss

    def set(self, idx=None):
        """Queue behind update(): the slots of the draw (self.idx, or `idx`: the ring's slots, never the staged positions of an
        n-step fold) get the priorities of self.td; td < 0 and idx < 0 leave their leaf as it was.  One launch."""
        if self.batch_size == 0:
            raise RuntimeError("set() without a draw")
        idx = self.idx if idx is None else self._rows(idx, self.torch.int32, "idx")
        self._set(self.tree, self.pmax, idx, self.td)

    def _warm_up(self, view=None):
        """Every kernel of the four calls once, and no trace: insert, draw and set run on a scratch tree with a scratch pmax,
        a scratch header and scratch outputs; the update (with view=) gets a draw without a sample, which is documented to
        write nothing but loss, grad and td, and those are put back."""
        torch, lb, dev = self.torch, self.learners, self.device
        if self.batch_size == 0:
            raise RuntimeError("_warm_up() before the buffers of a batch size exist: call _grow(B)")
        tree, pmax = self._tree(), self._pmax()
        header = torch.zeros_like(self.ring.header)
        idx, weight, q = torch.full_like(self.idx, -1), torch.zeros_like(self.weight), torch.zeros_like(self._q)
        self._insert(tree, pmax, header)
        self._draw(tree, idx, weight, q)
        self._set(tree, pmax, idx, torch.full_like(self.td, -1.0))
        if view is not None:
            loss, grad, td = lb.loss.clone(), lb.grad.clone(), self.td.clone()
            self.update(view, self.batch_size, torch.full_like(self.idx, -1))
            lb.loss.copy_(loss)
            lb.grad.copy_(grad)
            self.td.copy_(td)

    # ------------------------------------------------------------------ reading and resuming
    def levels(self):
        """the trees as numpy arrays (a host read): [leaves uint32 [P][n_0], uint64 [P][n_1], ..., the roots uint64 [P][1]]"""
        raw = self.tree.cpu().numpy()
        out, P = [], self.networks
        for k in range(self.layout["levels"]):
            n, stride, off = self.layout["n"][k], self.layout["stride"][k], self.layout["offset"][k]
            dtype = np.uint32 if k == 0 else np.uint64
            rows = raw[off:off + P * stride * np.dtype(dtype).itemsize].view(dtype).reshape(P, stride)
            out.append(rows[:, :n].copy())
        return out

    def state_dict(self):
        return {"tree": self.tree.detach().cpu().clone(), "pmax": self.pmax.detach().cpu().clone(),
                "hyper": {"alpha": self.alpha, "beta0": self.beta0, "anneal": self.anneal, "eps": self.eps, "shape": list(self._shape)}}

    def load_state_dict(self, state):
        """Resume bit for bit: the trees and pmax (with the learner bank's and the ring's own states, the next draw is the
        one the saved object would have made)."""
        torch = self.torch
        h = state.get("hyper", {})
        if list(h.get("shape", self._shape)) != list(self._shape):
            raise ValueError("the state was saved with (capacity, N, seg, P) = %r, this object has %r" % (h.get("shape"), self._shape))
        for name in ("tree", "pmax"):
            src, dst = torch.as_tensor(state[name]), getattr(self, name)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name, dst.dtype, tuple(dst.shape)))
        self.tree.copy_(torch.as_tensor(state["tree"]))
        self.pmax.copy_(torch.as_tensor(state["pmax"]))
        self.alpha, self.beta0 = float(h.get("alpha", self.alpha)), float(h.get("beta0", self.beta0))
        self.anneal, self.eps = int(h.get("anneal", self.anneal)), float(h.get("eps", self.eps))
        return self
