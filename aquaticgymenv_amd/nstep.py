"""Multi-step returns on the device: the n-step fold of the experience ring (libaqua_nstep.so, csrc/aqua_nstep.h).

The learners compute the one-step TD target of main/impl/dqn.py:262-292, y = r + gamma f(s') (masked by done).  An n-step
target, y = sum_{k<L} gamma^k r_{t+k} + gamma^n f(s_{t+n}), is the same formula on another transition: (s_t, a_t, R, s_{t+L},
d_{t+L-1}) with the discount gamma^n.  NStepReturns stages exactly that for every sample of a draw, in ONE launch, and
derives gamma^n beside it -- for a learner bank from its device table, so that a gamma PBT has just perturbed is already the
one this iteration bootstraps with.  The learners are then called unchanged:

    idx = ring.draw(B, learner, out=idx)
    nstep.fold(idx, gamma=learner.gamma)
    learner.update(nstep.view, B, idx=nstep.idx, gamma=nstep.discount(learner.gamma))

    learners.draw(ring, B, out=idx)
    nstep.fold(idx, hyper=learners.hyper)
    learners.update(nstep.view, B, nstep.idx, hyper=nstep.hyper)

A window is the transitions of ONE world: with the ring's capacity a multiple of env.num_envs, the next step of the world
in slot c is slot c + num_envs (mod capacity).  It ends at the first episode end; a window that would run past the newest
round, or that meets a step that is no experience, is no sample (the learners skip it as they skip idx == -1).  With n = 1
the staged rows are the ring's rows of the drawn slots bit for bit.  There is no CPU path.
"""
import ctypes


class _StagedView(object):
    """what DQNLearner.update(view, B, idx=...) and DQNLearnerBank.update(view, B, idx, ...) read of the staged minibatch:
    the six tensors, and capacity = size = P * B (what replay._LearnerView is to the ring)"""

    def __init__(self, rows, samples):
        self.s, self.a, self.r, self.s2, self.d, self.ok = rows
        self.capacity = self.size = samples


class NStepReturns(object):
    def __init__(self, ring, n, batch_size, networks=1):
        """ring: a DeviceReplayRing whose capacity is a multiple of its env's num_envs; n: the window, 1 .. MAX_STEPS;
        batch_size: samples per network and fold; networks: P, the rows of the draw (1 for a DQNLearner, the bank's number
        of networks for a DQNLearnerBank).  Anything else is a ValueError.  Owns the staged rows (s, s2 float32 [5][P B];
        r float32; a uint8, or float32 [2][P B] for continuous worlds; d, ok, length uint8), idx int32 [P][B] = p B + j (the
        constant draw that names every staged sample), hyper float64 [P][8] (the bank's table with gamma^n in word 0, written
        by fold(hyper=)) and view, the staged rows as the learners read a ring."""
        if getattr(ring, "header", None) is None or not hasattr(ring, "env"):
            raise ValueError("expected a DeviceReplayRing")
        torch = ring.torch
        if ring.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("NStepReturns runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (ring.device,))
        from . import _nstep_capi                     # (lazily: nothing else depends on libaqua_nstep.so)
        self._capi = _nstep_capi
        n, B, P = int(n), int(batch_size), int(networks)
        if not 1 <= n <= _nstep_capi.MAX_STEPS:
            raise ValueError("n=%d: must be in [1, %d]" % (n, _nstep_capi.MAX_STEPS))
        if not 1 <= B <= _nstep_capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [1, %d]" % (B, _nstep_capi.MAX_BATCH))
        if not 1 <= P <= _nstep_capi.MAX_NETWORKS:
            raise ValueError("networks=%d: must be in [1, %d]" % (P, _nstep_capi.MAX_NETWORKS))
        if ring.capacity % ring.env.num_envs != 0:
            raise ValueError("the ring's capacity (%d) must be a multiple of the batch (%d worlds): the next step of a world is then "
                             "the slot one batch further" % (ring.capacity, ring.env.num_envs))
        self.torch, self.ring, self.device = torch, ring, ring.device
        self.n, self.batch_size, self.networks, self.samples = n, B, P, P * B
        self.idx = torch.arange(P * B, dtype=torch.int32, device=self.device).reshape(P, B)
        self.hyper = torch.zeros((P, _nstep_capi.HYPER_WORDS), dtype=torch.float64, device=self.device)
        self._rows = self._staging()
        self.s, self.a, self.r, self.s2, self.d, self.ok, self.length = self._rows
        self.view = _StagedView(self._rows[:6], P * B)

    # ------------------------------------------------------------------ plumbing
    def _staging(self):
        """-> (s, a, r, s2, d, ok, length), zeroed, with the pitch P * B"""
        torch, dev, m = self.torch, self.device, self.samples
        a = torch.zeros((2, m), dtype=torch.float32, device=dev) if self.ring.env.continuous else torch.zeros(m, dtype=torch.uint8, device=dev)
        return (torch.zeros((5, m), dtype=torch.float32, device=dev), a, torch.zeros(m, dtype=torch.float32, device=dev),
                torch.zeros((5, m), dtype=torch.float32, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev),
                torch.zeros(m, dtype=torch.uint8, device=dev), torch.zeros(m, dtype=torch.uint8, device=dev))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _launch(self, idx, gamma, hyper, rows, hyper_out):
        """aquanst_fold on the ring: idx int32 [P][B]; gamma a float or hyper a table; rows: the seven staged tensors"""
        ring, capi = self.ring, self._capi
        s, a, r, s2, d, ok, length = rows
        with self.torch.cuda.device(self.device):
            rc = capi.lib.aquanst_fold(
                ring.header.data_ptr(), ring.s.data_ptr(), ring.a.data_ptr(), ring.r.data_ptr(), ring.s2.data_ptr(), ring.d.data_ptr(),
                ring.ok.data_ptr(), ring.capacity, ring.capacity, ring._kind, ring.env.num_envs,
                idx.data_ptr(), self.networks, self.batch_size, self.n,
                capi.NO_GAMMA if hyper is not None else float(gamma), None if hyper is None else hyper.data_ptr(),
                s.data_ptr(), a.data_ptr(), r.data_ptr(), s2.data_ptr(), d.data_ptr(), ok.data_ptr(), self.samples,
                length.data_ptr(), None if hyper is None else hyper_out.data_ptr(), self._stream())
        capi.check(rc, "aquanst_fold")

    # ------------------------------------------------------------------ the path
    def fold(self, idx, gamma=None, hyper=None):
        """Queue the fold of the draw `idx` (int32 [P][B], or [B] for one network: slots of the ring, -1 for none) on torch's
        current stream: one launch, no allocation, no host read.  Exactly one of gamma (a float, the learner's) and hyper (a
        learner bank's device table, float64 [P][8]); with hyper, self.hyper receives the table with gamma_p^n in word 0.
        -> self.view"""
        torch, P, B = self.torch, self.networks, self.batch_size
        if (gamma is None) == (hyper is None):
            raise ValueError("pass exactly one of gamma= (a float) and hyper= (a learner bank's device table)")
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.device != self.device or not idx.is_contiguous() \
                or tuple(idx.shape) not in (((P, B),) if P > 1 else ((P, B), (B,))):
            raise ValueError("idx must be a contiguous int32 [%d][%d] tensor on %s" % (P, B, self.device))
        if hyper is not None and (not isinstance(hyper, torch.Tensor) or hyper.dtype != torch.float64 or hyper.device != self.device
                                  or tuple(hyper.shape) != (P, self._capi.HYPER_WORDS) or not hyper.is_contiguous()):
            raise ValueError("hyper must be a contiguous float64 [%d][%d] tensor on %s" % (P, self._capi.HYPER_WORDS, self.device))
        self._launch(idx, gamma, hyper, self._rows, self.hyper)
        return self.view

    def discount(self, gamma):
        """aquanst_discount(gamma, n) on the host: what to pass to DQNLearner.update(..., gamma=) with the staged rows"""
        return self._capi.discount(gamma, self.n)

    def _warm_up(self, with_table):
        """the fold's kernel once, on scratch rows and a draw without a sample: the staged rows and self.hyper keep their bytes"""
        torch = self.torch
        idx = torch.full_like(self.idx, -1)
        if with_table:
            table = torch.zeros_like(self.hyper)
            self._launch(idx, None, table, self._staging(), torch.zeros_like(self.hyper))
        else:
            self._launch(idx, 0.0, None, self._staging(), None)
