"""EvolutionStrategy: natural evolution strategies (Salimans et al. 2017) on a QNetworkBank, on the device by libaqua_evo.so
(csrc/aqua_evo.h) -- the gradient-free, population-based counterpart of the DQN learners.

A bank of P = 2H networks holds the antithetic perturbations theta +- sigma eps of one centre theta (an odd P keeps the centre
itself in the last slot, which shows the centre's own fitness for free).  Every member flies its own segment of `bank.seg`
worlds, one episode per world; the members are ranked by mean return or success rate, and the centre takes one Adam or SGD
step along sum (rank difference) eps.  No replay ring, no TD target, no backward pass: what is optimised is the quantity
Policy.test / run_tests report.

    es = EvolutionStrategy(bank, sigma=0.05, lr=0.01, seed=1)
    for _ in range(generations):
        es.generation(env)             # ask(), evaluate(env), tell()

The noise is never stored: ask() and tell() regenerate it from Philox, keyed by (seed, generation, pair, parameter), as an
Irwin-Hall sum of eight 16-bit uniforms with an integer numerator -- isotropic, unit variance, and NOT a Gaussian.  All state
is device memory (theta, m, v, the step counter and a header with the generation); ask() is one launch, fitness() three and
tell() two, with no allocation, no synchronisation and no host read: each works unchanged inside torch.cuda.graph (a graph
keeps the sigma, lr and seed of its capture).  Only evaluate()'s poll of the episode counter, centre_layers(), report() and
state_dict() read back.  There is no CPU path.
"""
import ctypes
import math

import numpy as np

_SCORES = {"mean_return": 0, "success_rate": 1}
_OPTIMIZERS = {"adam": 0, "sgd": 1}
_MASK = (1 << 64) - 1


class EvolutionStrategy(object):
    def __init__(self, bank, centre=None, sigma=0.05, lr=0.01, seed=0, optimizer="adam", betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, score="mean_return", actor=None):
        """bank: the QNetworkBank whose P slots hold the population (P even: all perturbed; P odd: the last slot acts with the
        centre).  centre: a layer stack [(kernel, bias)] * 3, a QNetwork, or None for the layers slot 0 holds now.  sigma: the
        perturbation's scale, > 0; lr, betas, eps, weight_decay, optimizer ("adam" or "sgd"): the centre's optimiser.
        score: "mean_return" or "success_rate".  actor: a FastActor over the bank, refreshed behind every ask()."""
        from .fastpolicy import FastActor
        from .qbank import QNetworkBank
        from .qpolicy import QNetwork
        if not isinstance(bank, QNetworkBank):
            raise ValueError("expected a QNetworkBank")
        from . import _evo_capi, _learner_capi        # (lazily: nothing else depends on libaqua_evo.so)
        self._capi = _evo_capi
        if bank.networks > _evo_capi.MAX_NETWORKS:
            raise ValueError("the bank holds %d networks, an EvolutionStrategy steps at most %d" % (bank.networks, _evo_capi.MAX_NETWORKS))
        if actor is not None and (not isinstance(actor, FastActor) or actor.source is not bank):
            raise ValueError("actor: expected a FastActor over this bank")
        torch = bank.torch
        self.torch, self.bank, self.device, self.actor = torch, bank, bank.device, actor
        self.networks = P = bank.networks
        self.pairs = P // 2
        self.seg = bank.seg
        self._configure(sigma, lr, seed, optimizer, betas, eps, weight_decay, score)
        if centre is None:
            layers = bank.layers[0]
        elif isinstance(centre, QNetwork) and not isinstance(centre, QNetworkBank):
            layers = centre.layers
        else:
            layers = centre
        theta = _learner_capi.flatten(layers)
        dev = self.device
        slot_bytes = int(bank.tensor.shape[1])
        if slot_bytes % 16 != 0:
            raise RuntimeError("the bank's slot of %d bytes is no multiple of 16: rebuild" % slot_bytes)
        self.blob_floats = slot_bytes // 4
        self.theta = torch.from_numpy(theta.copy()).to(dev)
        self.m = torch.zeros(_evo_capi.PARAMS, dtype=torch.float32, device=dev)
        self.v = torch.zeros(_evo_capi.PARAMS, dtype=torch.float32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)                                   # the library's uint64 [1]
        self.header = torch.zeros(_evo_capi.HEADER, dtype=torch.int64, device=dev)               # the library's uint64 [8]
        self.perm = torch.from_numpy(_learner_capi.permutation()).to(dev)
        self.fitness_out = torch.full((P,), float("-inf"), dtype=torch.float32, device=dev)
        self.episodes = torch.zeros(P, dtype=torch.int64, device=dev)
        self.acc = torch.zeros((P, _evo_capi.ACC), dtype=torch.int64, device=dev)
        self.rank2 = torch.zeros(max(2 * self.pairs, 1), dtype=torch.int32, device=dev)
        self.weights = torch.zeros(max(self.pairs, 1), dtype=torch.int32, device=dev)
        self.tracker = None

    def _configure(self, sigma, lr, seed, optimizer, betas, eps, weight_decay, score):
        try:
            beta1, beta2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas: two numbers, got %r" % (betas,)) from None
        sigma, lr, eps, weight_decay = float(sigma), float(lr), float(eps), float(weight_decay)
        if not (math.isfinite(sigma) and sigma > 0.0):
            raise ValueError("sigma=%r: must be finite and > 0" % (sigma,))
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError("lr=%r: must be finite and >= 0" % (lr,))
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError("betas=%r: both must be in [0, 1)" % ((beta1, beta2),))
        if not (math.isfinite(eps) and eps > 0.0):
            raise ValueError("eps=%r: must be finite and > 0" % (eps,))
        if not (math.isfinite(weight_decay) and weight_decay >= 0.0):
            raise ValueError("weight_decay=%r: must be finite and >= 0" % (weight_decay,))
        if optimizer not in _OPTIMIZERS:
            raise ValueError("optimizer %r: one of %s" % (optimizer, sorted(_OPTIMIZERS)))
        if score not in _SCORES:
            raise ValueError("score %r: one of %s" % (score, sorted(_SCORES)))
        self.sigma, self.lr, self.betas, self.eps, self.weight_decay = sigma, lr, (beta1, beta2), eps, weight_decay
        self.optimizer, self.score, self.seed = optimizer, score, int(seed) & _MASK

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _ask(self, theta, header, P, sigma, blob):
        with self.torch.cuda.device(self.device):
            rc = self._capi.lib.aquaevo_ask(theta.data_ptr(), self.perm.data_ptr(), header.data_ptr(), P, sigma, self.seed,
                                            blob.data_ptr(), self.blob_floats, self._stream())
        self._capi.check(rc, "aquaevo_ask")

    def _fitness(self, tracker, counts, acc, fitness, episodes):
        unfinished = tracker.finished is not None
        with self.torch.cuda.device(self.device):
            rc = self._capi.lib.aquaevo_fitness(
                tracker.log_ret.data_ptr(), tracker.log_code.data_ptr(), tracker.log_world.data_ptr(), tracker.capacity, counts.data_ptr(),
                tracker.ret.data_ptr() if unfinished else None, tracker.finished.data_ptr() if unfinished else None,
                int(tracker.env.env_offset), tracker.num_envs, self.seg, self.networks, _SCORES[self.score],
                acc.data_ptr(), fitness.data_ptr(), episodes.data_ptr(), self._stream())
        self._capi.check(rc, "aquaevo_fitness")

    def _tell(self, fitness, header, theta, m, v, t, rank2, weights, grad_out=None):
        with self.torch.cuda.device(self.device):
            rc = self._capi.lib.aquaevo_tell(
                fitness.data_ptr(), self.networks, header.data_ptr(), theta.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(),
                self.sigma, self.seed, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, _OPTIMIZERS[self.optimizer],
                rank2.data_ptr(), weights.data_ptr(), None if grad_out is None else grad_out.data_ptr(), self._stream())
        self._capi.check(rc, "aquaevo_tell")

    def _check_tracker(self, tracker):
        from .episodes import EpisodeTracker
        if not isinstance(tracker, EpisodeTracker):
            raise ValueError("expected an EpisodeTracker")
        if tracker.device != self.device:
            raise ValueError("the tracker is on %s, the bank on %s" % (tracker.device, self.device))

    def _check_fitness(self, fitness):
        torch = self.torch
        if not isinstance(fitness, torch.Tensor) or fitness.dtype != torch.float32 or fitness.device != self.device or fitness.dim() != 1 \
                or fitness.numel() < self.networks or not fitness.is_contiguous():
            raise ValueError("fitness must be a contiguous float32 [>=%d] tensor on %s" % (self.networks, self.device))

    # ------------------------------------------------------------------ the path
    def ask(self):
        """Fill the bank with this generation's population, queued on torch's current stream: one launch, and the actor's
        refresh behind it.  Slot 2j holds theta + sigma eps_j, slot 2j + 1 theta - sigma eps_j, the last slot of an odd bank
        the centre.  The bank's host copy `bank.layers` is stale from then on."""
        self._ask(self.theta, self.header, self.networks, self.sigma, self.bank.tensor)
        if self.actor is not None:
            self.actor.refresh()

    def fitness(self, tracker):
        """The score of every network from an EpisodeTracker's log (and, for a once=True tracker, the running returns of the
        worlds that have not ended), queued on torch's current stream: three launches.  -> the device float32 [P], owned by
        this object; `episodes` (int64 [P]) holds the episodes counted.  A network without an episode scores -infinity."""
        self._check_tracker(tracker)
        self._fitness(tracker, tracker._counts, self.acc, self.fitness_out, self.episodes)
        return self.fitness_out

    def tell(self, fitness=None):
        """One step of the centre from the fitness of the population asked last (default: what fitness() wrote), queued on
        torch's current stream: two launches.  Advances the generation."""
        fitness = self.fitness_out if fitness is None else fitness
        self._check_fitness(fitness)
        self._tell(fitness, self.header, self.theta, self.m, self.v, self.t, self.rank2, self.weights)

    def _warm_up(self, tracker=None):
        """every kernel once, on scratch buffers: no trace is left in the bank, the centre, the header or the outputs"""
        torch, dev = self.torch, self.device
        self._ask(self.theta, torch.zeros_like(self.header), 1, self.sigma, torch.zeros(self.blob_floats, dtype=torch.float32, device=dev))
        if self.actor is not None:
            self.actor.refresh()
        if tracker is not None:
            self._check_tracker(tracker)
            self._fitness(tracker, torch.zeros_like(tracker._counts), torch.zeros_like(self.acc), torch.zeros_like(self.fitness_out),
                          torch.zeros_like(self.episodes))
        self._tell(torch.zeros_like(self.fitness_out), torch.zeros_like(self.header), self.theta.clone(), self.m.clone(), self.v.clone(),
                   torch.zeros_like(self.t), torch.zeros_like(self.rank2), torch.zeros_like(self.weights))

    def evaluate(self, env, max_steps=1001, poll=64):
        """One episode per world of a discrete auto_reset=False batch of bank.seg worlds per network: env.reset(), then
        episodes.evaluate()'s loop under env.step(policy=bank) (the actor, if there is one) with a once=True tracker, then
        fitness().  The only host read is the poll of the episode counter.  -> the device float32 [P] of fitness()."""
        from .episodes import EpisodeTracker
        if int(env.auto_reset) != 0:
            raise ValueError("evaluate(): one episode per world needs an auto_reset=False batch")
        if getattr(env, "continuous", False):
            raise ValueError("the Q-network policy (main/impl/dqn.py) is defined for discrete actions")
        n = int(env.num_envs)
        if n != self.networks * self.seg:
            raise ValueError("the batch has %d worlds, the bank %d networks of %d" % (n, self.networks, self.seg))
        if self.tracker is None or self.tracker.env is not env:
            self.tracker = EpisodeTracker(env, capacity=n, once=True)
        else:
            self.tracker.reset_stats()
        tracker, policy = self.tracker, self.bank if self.actor is None else self.actor
        env.reset()
        poll = max(int(poll), 1)
        for step in range(int(max_steps)):
            env.step(policy=policy)
            tracker.after_step()
            if step % poll == poll - 1 and tracker.counts()["episodes"] == n:
                break
        return self.fitness(tracker)

    def generation(self, env, max_steps=1001, poll=64):
        """ask(), evaluate(env), tell() -> the device fitness of the generation just flown"""
        self.ask()
        fitness = self.evaluate(env, max_steps, poll)
        self.tell()
        return fitness

    def write_centre(self, qnet):
        """The centre into a QNetwork's blob (an ask with P = 1), queued on torch's current stream.  qnet.layers is stale
        from then on.  -> qnet"""
        from .qbank import QNetworkBank
        from .qpolicy import QNetwork
        if not isinstance(qnet, QNetwork) or isinstance(qnet, QNetworkBank) or getattr(qnet, "source", None) is not None:
            raise ValueError("expected a QNetwork or a bank.view(p)")
        if qnet.device != self.device or int(qnet.blob.numel()) != 4 * self.blob_floats:
            raise ValueError("the network is on %s with a blob of %d bytes, the bank on %s with slots of %d" %
                             (qnet.device, int(qnet.blob.numel()), self.device, 4 * self.blob_floats))
        self._ask(self.theta, self.header, 1, self.sigma, qnet.blob)
        return qnet

    # ------------------------------------------------------------------ reading (host reads)
    def centre_layers(self):
        """the centre as a layer stack [(kernel, bias)] * 3"""
        from . import _learner_capi
        return _learner_capi.unflatten(self.theta.cpu().numpy())

    def report(self):
        """-> {"generation", "tells", "stepped", "best", "ranked", "t", "fitness", "episodes"}: the generation the next ask
        draws, tell() calls so far, the generation the last tell stepped with, the best ranked slot of the last tell (None
        before it, or with one network), the slots it ranked, the optimiser's step counter, and what fitness() wrote last"""
        h = [int(x) for x in self.header.cpu().numpy().view(np.uint64)]
        c = self._capi
        best = h[c.H_BEST]
        return {"generation": h[c.H_GENERATION], "tells": h[c.H_TELLS], "stepped": h[c.H_STEPPED],
                "best": None if best == c.NO_SLOT or h[c.H_TELLS] == 0 else best, "ranked": h[c.H_RANKED],
                "t": int(self.t.cpu().numpy().view(np.uint64)[0]), "fitness": self.fitness_out.cpu().numpy().copy(),
                "episodes": self.episodes.cpu().numpy().copy()}

    # ------------------------------------------------------------------ resuming
    _STATE = ("theta", "m", "v", "t", "header")
    _CONFIG = ("sigma", "lr", "seed", "optimizer", "betas", "eps", "weight_decay", "score")

    def state_dict(self):
        """theta, m, v, t, the header and the configuration"""
        out = {name: getattr(self, name).detach().cpu().clone() for name in self._STATE}
        out["config"] = dict({name: getattr(self, name) for name in self._CONFIG}, networks=self.networks)
        return out

    def load_state_dict(self, state):
        """Resume bit for bit: the centre, the moments, the counters and the configuration (the saved one wins)."""
        torch = self.torch
        config = dict(state.get("config", {}))
        if config.pop("networks", self.networks) != self.networks:
            raise ValueError("the state was saved with another number of networks than this bank's %d" % self.networks)
        for name in self._STATE:
            src, dst = torch.as_tensor(state[name]), getattr(self, name)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("state[%r]: expected %s %s" % (name, dst.dtype, tuple(dst.shape)))
        self._configure(**dict({name: getattr(self, name) for name in self._CONFIG}, **config))
        for name in self._STATE:
            getattr(self, name).copy_(torch.as_tensor(state[name]))
        return self
