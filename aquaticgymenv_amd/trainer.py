"""DQNLoop: one iteration of the reference's training loop (main/impl/dqn.py:147-184) as ONE chain of launches on one
stream, and that chain captured into one HIP graph.

Every stage already lives on the device -- the Q-network policy (qpolicy.py), the exploration pass and the episode
accounting (episodes.py), the step kernels (batched.py), the learner (learner.py) -- and each is capturable by itself.  What
kept the whole iteration out of a graph was the experience ring's cursor and size, Python integers of ReplayRing;
DeviceReplayRing (replay.py) keeps them in device memory.  An iteration is then, in stream order:

    1. greedy policy launch, keyed by the device tick base      6. tracker.after_step()         (two launches)
    2. tracker.explore(tick_base=...)                           7. ring draw: idx of the update t -> t + 1
    3. ring open: (s, a, ok)                                    8. learner.update(view, B, idx=idx)  (two launches)
    4. step launch                                              9. tick advance
    5. ring close: (r, s', d), cursor and size move on

step() queues exactly that eagerly; capture() records the same calls once and launch() replays them: eleven kernels, no
host work between them.  With actor=, a FastActor (fastpolicy.py) over the acting network, stage 1 launches it and its
refresh() follows stage 8: twelve kernels.  Both give, bit for bit, what examples/dqn_train.py --eager computes with ReplayRing and
learner.update(ring, B).  With n_step > 1, an NStepReturns (nstep.py) folds the draw between stages 7 and 8 -- one kernel more in
either variant, twelve or thirteen -- and the update learns the n-step target from its staged rows with the discount
gamma^n; n_step = 1 is the chain above, node for node.  With hindsight=, a HindsightReplay (hindsight.py) relabels the draw
between stages 7 and 8 -- one kernel more -- and the update learns from its staged rows; hindsight=None is the chain above,
node for node.  There is no CPU path.
"""
import ctypes

from . import _capi, _learner_capi
from .batched import RolloutGraph


class DQNLoop(object):
    def __init__(self, env, qnet, learner, ring, tracker, batch_size=64, actor=None, n_step=1, hindsight=None):
        """env: a BatchedAqua of discrete actions with normalized_obs=True; qnet: the acting QNetwork; learner: the DQNLearner
        that trains it; ring: a DeviceReplayRing of env; tracker: an EpisodeTracker of env with an epsilon schedule;
        actor: None, or a FastActor (fastpolicy.py) over qnet -- the act stage then launches it, and one actor.refresh()
        follows the update: one kernel more, eagerly and in the graph.  n_step: 1, or the window of an n-step target
        (nstep.py): one fold launch then goes between the draw and the update, and the ring's capacity must be a multiple of
        env.num_envs.  The discount gamma^n is passed to the update by value: a graph keeps the one of its capture.
        hindsight: None, or a HindsightReplay (hindsight.py) of `ring` for one network and this batch size: its launch goes
        between the draw and the update.  Not together with n_step > 1 (every step of a window would need its reward
        recomputed).
        Everything on one device; anything else is a ValueError."""
        if env.continuous:
            raise ValueError("the DQN loop (main/impl/dqn.py) is defined for discrete actions")
        if env.obs_norm_buf is None:
            raise ValueError("the ring stores the normalised observation: construct the env with normalized_obs=True")
        if not getattr(qnet, "_aquapol_network", False):
            raise ValueError("expected a QNetwork")
        if learner.qnet is not qnet:
            raise ValueError("the learner trains another network than the one that acts")
        if getattr(ring, "header", None) is None or ring.env is not env:
            raise ValueError("expected a DeviceReplayRing of this env")
        if tracker.env is not env or tracker.epsilon is None:
            raise ValueError("expected an EpisodeTracker of this env with epsilon=(init, final, decay)")
        for what, dev in (("network", qnet.device), ("learner", learner.device), ("ring", ring.device), ("tracker", tracker.device)):
            if dev != env.device:
                raise ValueError("the environment is on %s, the %s on %s" % (env.device, what, dev))
        B = int(batch_size)
        if B < 1 or B > _learner_capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [1, %d]" % (B, _learner_capi.MAX_BATCH))
        self.actor = self._check_actor(actor, qnet)
        self.env, self.qnet, self.learner, self.ring, self.tracker, self.batch_size = env, qnet, learner, ring, tracker, B
        self.torch = env.torch
        self.view = ring.learner_view()
        self.idx = self.torch.full((B,), -1, dtype=self.torch.int32, device=env.device)
        self.nstep = self._make_nstep(ring, n_step, B, 1)
        self.hindsight = self._check_hindsight(hindsight, ring, B, 1)
        env.policy_action                                     # (allocated here, not inside a capture)
        learner._grow(B)

    def _make_nstep(self, ring, n_step, B, networks):
        """n_step == 1: None, nothing is built; otherwise the NStepReturns of this loop"""
        self.n_step = int(n_step)
        if self.n_step == 1:
            return None
        from .nstep import NStepReturns
        return NStepReturns(ring, self.n_step, B, networks=networks)

    def _check_hindsight(self, hindsight, ring, B, networks, priorities=None):
        """hindsight=: None, or a HindsightReplay of this ring, batch size and number of networks; nothing is built here"""
        if hindsight is None:
            return None
        if not hasattr(hindsight, "relabel") or not hasattr(hindsight, "_warm_up"):
            raise ValueError("hindsight= must be a HindsightReplay")
        if self.n_step != 1:
            raise ValueError("hindsight= together with n_step=%d: every step of a window would need its reward recomputed under "
                             "the new goal; use one of them" % self.n_step)
        if priorities is not None:
            raise ValueError("hindsight= together with priorities=: the TD error of a relabelled transition is not a priority of "
                             "the stored slot; use one of them")
        if hindsight.ring is not ring:
            raise ValueError("hindsight= relabels from another ring than the loop's")
        if hindsight.batch_size != B or hindsight.networks != networks:
            raise ValueError("hindsight= stages %d x %d samples, the loop draws %d x %d"
                             % (hindsight.networks, hindsight.batch_size, networks, B))
        return hindsight

    @staticmethod
    def _check_actor(actor, policy):
        """actor=: None, or a FastActor whose source is the loop's own network or bank"""
        if actor is not None and (not hasattr(actor, "refresh") or getattr(actor, "source", None) is not policy):
            raise ValueError("actor= must be a FastActor over the network (or bank) this loop trains")
        return actor

    def _act_fast(self, s):
        """the act stage through the FastActor: its library's checker, its entry's name and its message"""
        from . import _fastpol_capi
        env = self.env
        _fastpol_capi.check(env._policy_launch(self.actor, 0.0, 0, env._tick_dev.data_ptr(), s), "aquafast_act_f16")

    def _act(self, s):
        from . import _policy_capi
        if self.actor is not None:
            return self._act_fast(s)
        env = self.env
        _policy_capi.check(env._policy_launch(self.qnet, 0.0, 0, env._tick_dev.data_ptr(), s), "aquapol_act_f32")

    # ------------------------------------------------------------------ the iteration
    def _queue(self):
        """the nine stages on torch's current stream, every draw keyed by the device tick base"""
        env, ring, tracker = self.env, self.ring, self.tracker
        action, tb = env.policy_action, env._tick_dev
        s = env._stream()
        self._act(s)
        tracker.explore(action, tick=0, tick_base=tb)
        ring.before_step(action)
        _capi.check(env._step_launch(action.data_ptr(), _capi.ACT_U8, 0, 0, tb.data_ptr(), env.reward.data_ptr(),
                                     env.term.data_ptr(), env.done_bits.data_ptr(), s), "aqua_step_f32")
        ring.after_step()
        tracker.after_step()
        ring.draw(self.batch_size, self.learner, out=self.idx)
        if self.hindsight is not None:
            her = self.hindsight
            her.relabel(self.idx, self.learner)               # keyed by the learner's t, which the update below advances
            self.learner.update(her.view, self.batch_size, idx=her.idx)
        elif self.nstep is None:
            self.learner.update(self.view, self.batch_size, idx=self.idx)
        else:
            nstep, gamma = self.nstep, self.learner.gamma
            nstep.fold(self.idx, gamma=gamma)
            self.learner.update(nstep.view, self.batch_size, idx=nstep.idx, gamma=nstep.discount(gamma))
        if self.actor is not None:
            self.actor.refresh()                              # the next iteration acts with the weights of this update
        _capi.check(_capi.lib.aqua_tick_advance(tb.data_ptr(), 1, s), "aqua_tick_advance")

    def step(self):
        """Queue one iteration eagerly -> (reward, term) of its step, as env.step() returns them"""
        env = self.env
        with self.torch.cuda.device(env.device):
            env._sync_device_tick()
            self._queue()
        env._tick += 1
        env._device_tick += 1
        return env.reward[:env.num_envs], env.term[:env.num_envs]

    # ------------------------------------------------------------------ the graph
    def _warm_up(self):
        """Every kernel of the iteration runs once, on the current stream, and leaves no trace: the kernels' code is on the
        device before the capture begins.  The policy writes policy_action (an output); the exploration pass works on a
        scratch row; the accounting sees a batch in which no world counts; the ring kernels run on a one-slot scratch ring;
        the learner gets a minibatch without a sample (documented to leave everything as it was); the fold, if there is
        one, runs on scratch rows with a draw without a sample; the step is taken on a snapshot and taken back."""
        torch, env, tracker, learner = self.torch, self.env, self.tracker, self.learner
        dev, n = env.device, env.num_envs
        rpl = self.ring._capi
        s = env._stream()
        tb = env._tick_dev
        self._act(s)
        if self.actor is not None:
            self.actor.refresh()                              # (the weights have not changed: the same bytes again)
        tracker.explore(torch.zeros(env.ld, dtype=torch.uint8, device=dev), tick=0, tick_base=tb)
        tracker.after_step(torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                           torch.full((n,), -1, dtype=torch.int32, device=dev))
        header = torch.zeros(rpl.HEADER_WORDS, dtype=torch.int64, device=dev)
        rows = torch.zeros((5, 1), dtype=torch.float32, device=dev)
        f32, u8 = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(3, dtype=torch.uint8, device=dev)
        idx = torch.full((self.batch_size,), -1, dtype=torch.int32, device=dev)
        rpl.check(rpl.lib.aquarpl_open(header.data_ptr(), rows.data_ptr(), u8[0:].data_ptr(), u8[1:].data_ptr(), 1, 1, rows.data_ptr(), 1,
                                       u8[2:].data_ptr(), rpl.ACT_U8, 1, None, 1, s), "aquarpl_open")
        rpl.check(rpl.lib.aquarpl_close(header.data_ptr(), f32.data_ptr(), rows.data_ptr(), u8[0:].data_ptr(), 1, 1, f32.data_ptr(),
                                        rows.data_ptr(), 1, u8[2:].data_ptr(), 1, s), "aquarpl_close")
        rpl.check(rpl.lib.aquarpl_draw(header.data_ptr(), u8[1:].data_ptr(), 1, learner.t.data_ptr(), learner.seed, idx.data_ptr(),
                                       self.batch_size, s), "aquarpl_draw")
        idx.fill_(-1)
        if self.nstep is not None:
            self.nstep._warm_up(with_table=False)
        if self.hindsight is not None:
            self.hindsight._warm_up(with_table=False)
        loss = learner.loss.clone()
        grad = learner.grad.clone()
        learner.update(self.view, self.batch_size, idx=idx)                  # no sample: nothing but loss and grad is written
        learner.loss.copy_(loss)
        learner.grad.copy_(grad)
        snap = env.snapshot()
        _capi.check(env._step_launch(env.policy_action.data_ptr(), _capi.ACT_U8, 0, 0, tb.data_ptr(), env.reward.data_ptr(),
                                     env.term.data_ptr(), env.done_bits.data_ptr(), s), "aqua_step_f32")
        env.restore(snap)
        _capi.check(_capi.lib.aqua_tick_advance(tb.data_ptr(), 0, s), "aqua_tick_advance")
        torch.cuda.current_stream(dev).synchronize()

    def capture(self):
        """-> a RolloutGraph whose launch() replays one iteration: the nine stages as ONE chain of eleven kernel nodes (no
        parallel branches; one node more with an actor, one more with n_step > 1 or with hindsight=).  It reads and advances the device state only -- tick base, epsilon, ring header, Adam's t -- so
        every replay acts, explores, appends, draws and learns afresh; qnet.load() or learner.load_state_dict() between
        replays takes effect on the next one.  The learner's workspace is grown and every kernel has run before the capture."""
        torch, env, lib = self.torch, self.env, _capi.lib
        with torch.cuda.device(env.device):
            env._sync_device_tick()
            self._warm_up()
            env._sync_device_tick()
            cap = torch.cuda.Stream(device=env.device)
            cap.wait_stream(torch.cuda.current_stream(env.device))
            handle = ctypes.c_void_p()
            was_open = self.ring._open
            try:
                with torch.cuda.stream(cap):
                    s = env._stream()
                    _capi.check(lib.aqua_graph_begin(s), "aqua_graph_begin")
                    error = None
                    try:
                        self._queue()
                    except Exception as exc:              # the capture must be ended before anything else happens
                        error = exc
                    rc_end = lib.aqua_graph_end(s, ctypes.byref(handle))
                    if error is not None:
                        if rc_end == 0:
                            lib.aqua_graph_destroy(handle)
                        self.ring._open = was_open
                        raise error
                    _capi.check(rc_end, "aqua_graph_end")
            finally:
                torch.cuda.current_stream(env.device).wait_stream(cap)
        g = RolloutGraph(env, handle, 1, env.reward, env.term)
        g._actions = (self.actor or self.qnet, env.policy_action)
        g._loop = self                                        # the buffers the graph's nodes point at
        g.done_history = None
        return g


class PopulationLoop(DQNLoop):
    """One iteration of P trainings on ONE batch of worlds as one chain of launches: the networks of a QNetworkBank act on
    their segments of the batch, the one ring records the step, and a DQNLearnerBank (lbank.py) draws every network's
    minibatch from its own slots and updates every network.  In stream order:

        1. bank act with the bank's device epsilon array, keyed by the device tick base
        2. ring open: (s, a, ok)                      5. tracker.after_step()               (two launches)
        3. step launch                                6. bank draw: idx [P][B] of the updates t_p -> t_p + 1
        4. ring close: (r, s', d)                     7. bank update                        (two launches)
                                                      8. tick advance

    Ten kernels.  step() queues them eagerly; capture().launch() replays them as ONE graph (DQNLoop's capture).  Network p
    explores with bank.epsilon[p], the caller's device array: the graph reads whatever it holds when it runs.  The tracker's
    log names the world of every episode, so the success rate of network p is that of the records with
    log_world // bank.seg == p.

    With segments=, a SegmentTracker (segments.py) of this tracker whose epsilon array IS bank.epsilon, stage 5 is followed by
    its launch: every network's schedule advances by the episodes its worlds finished in this step (dqn.py:184), and its
    counters and windowed statistics follow, on the device.  Eleven kernels, and no host read is needed to keep the loop
    correct.

    With selector=, a PopulationSelector (pbt.py) of these learners and this SegmentTracker, its two launches follow the
    SegmentTracker's and precede the draw: thirteen kernels.  A network replaced in an iteration is trained on its parent's
    weights by the update of that same iteration.

    With actor=, a FastActor (fastpolicy.py) over the bank, stage 1 is its launch and its refresh() follows the bank update:
    one kernel more in every variant above.

    With n_step > 1, an NStepReturns (nstep.py) folds the draw between stages 6 and 7: one kernel more in every variant above.
    It reads learners.hyper and writes its own table with gamma_p^n in word 0, which the bank update of the same iteration
    reads: after the selector has perturbed a gamma, that iteration already bootstraps with the new gamma^n, and no host read
    is involved.  n_step = 1 is the chain above, node for node.

    With priorities=, a PrioritizedReplay (priority.py) of this ring and these learners, replay is prioritised: its insert()
    follows stage 4, its draw() (two launches) is stage 6, its update() (two launches) is stage 7 and its set() follows it --
    three kernels more in every variant above.  With n_step > 1 the fold takes the draw's slots, the update the staged rows, and
    set() the draw's slots again; a window the fold dropped keeps its priority.  priorities=None is the chain above, node for
    node.

    With hindsight=, a HindsightReplay (hindsight.py) of this ring for the bank's networks, its launch relabels the draw between
    stages 6 and 7, keyed by the learners' device counters and keys, and the bank update reads its staged rows: one kernel
    more.  Not together with n_step > 1 or priorities=.  hindsight=None is the chain above, node for node.  There is no CPU
    path."""

    def __init__(self, env, bank, learners, ring, tracker, batch_size=64, segments=None, selector=None, actor=None, n_step=1,
                 priorities=None, hindsight=None):
        """env: a BatchedAqua of discrete actions with normalized_obs=True; bank: the acting QNetworkBank with its epsilon
        array set; learners: the DQNLearnerBank that trains it; ring: a DeviceReplayRing of env whose capacity is a multiple
        of env.num_envs; tracker: an EpisodeTracker of env; segments: None, or a SegmentTracker of that tracker with the
        bank's segment size and number of networks, whose epsilon is bank.epsilon; selector: None, or a PopulationSelector
        of `learners` and `segments`; actor: None, or a FastActor (fastpolicy.py) over `bank` -- the act stage then launches it
        and one actor.refresh() follows the bank update (which follows the selector when there is one): one kernel more.
        n_step: 1, or the window of an n-step target (nstep.py): one fold launch between the draw and the update.
        priorities: None, or a PrioritizedReplay (priority.py) of `ring` and `learners`: three kernels more.
        hindsight: None, or a HindsightReplay (hindsight.py) of `ring` for bank.networks networks and this batch size: one
        kernel more; not together with n_step > 1 or priorities=.
        Everything on one device; anything else is a ValueError."""
        from . import _lbank_capi
        if env.continuous:
            raise ValueError("the DQN loop (main/impl/dqn.py) is defined for discrete actions")
        if env.obs_norm_buf is None:
            raise ValueError("the ring stores the normalised observation: construct the env with normalized_obs=True")
        if not hasattr(bank, "networks") or not getattr(bank, "_aquapol_network", False):
            raise ValueError("expected a QNetworkBank")
        if getattr(learners, "bank", None) is not bank:
            raise ValueError("the learner bank trains another bank than the one that acts")
        if bank.epsilon is None:
            raise ValueError("set bank.epsilon to a float32 [networks] device tensor: every network explores with its own entry")
        if getattr(ring, "header", None) is None or ring.env is not env:
            raise ValueError("expected a DeviceReplayRing of this env")
        if tracker.env is not env:
            raise ValueError("expected an EpisodeTracker of this env")
        for what, dev in (("bank", bank.device), ("learner bank", learners.device), ("ring", ring.device), ("tracker", tracker.device)):
            if dev != env.device:
                raise ValueError("the environment is on %s, the %s on %s" % (env.device, what, dev))
        if ring.capacity % env.num_envs != 0:
            raise ValueError("the ring's capacity (%d) must be a multiple of the batch (%d worlds): a slot then belongs to one world, "
                             "and so to one network" % (ring.capacity, env.num_envs))
        if bank.seg * bank.networks < env.num_envs:
            raise ValueError("%d networks x %d worlds do not cover the batch of %d" % (bank.networks, bank.seg, env.num_envs))
        if segments is not None:
            if getattr(segments, "tracker", None) is not tracker:
                raise ValueError("expected a SegmentTracker of this EpisodeTracker")
            if segments.epsilon is None or segments.epsilon is not bank.epsilon:
                raise ValueError("set bank.epsilon = segments.epsilon: the bank explores with the schedules the SegmentTracker advances")
            if segments.seg != bank.seg or segments.segments != bank.networks:
                raise ValueError("the SegmentTracker has %d segments of %d worlds, the bank %d networks of %d" %
                                 (segments.segments, segments.seg, bank.networks, bank.seg))
        if selector is not None:
            if not hasattr(selector, "select") or not hasattr(selector, "_warm_up"):
                raise ValueError("expected a PopulationSelector")
            if segments is None or selector.segments is not segments:
                raise ValueError("the selector judges by another SegmentTracker than the loop's segments=")
            if selector.learners is not learners:
                raise ValueError("the selector selects among another learner bank than the one the loop trains")
        B = int(batch_size)
        if B < 1 or B > _lbank_capi.MAX_BATCH:
            raise ValueError("batch_size=%d: must be in [1, %d]" % (B, _lbank_capi.MAX_BATCH))
        self.env, self.bank, self.learners, self.ring, self.tracker, self.batch_size = env, bank, learners, ring, tracker, B
        self.segments, self.selector = segments, selector
        self.actor = self._check_actor(actor, bank)
        self.qnet = bank                                      # (what DQNLoop.capture() hands to the graph as its policy)
        self.torch = env.torch
        self.view = ring.learner_view()
        self.idx = self.torch.full((bank.networks, B), -1, dtype=self.torch.int32, device=env.device)
        self.nstep = self._make_nstep(ring, n_step, B, bank.networks)
        if priorities is not None:
            if not hasattr(priorities, "insert") or not hasattr(priorities, "_warm_up"):
                raise ValueError("expected a PrioritizedReplay")
            if priorities.ring is not ring or priorities.learners is not learners:
                raise ValueError("the PrioritizedReplay keeps the priorities of another ring or another learner bank")
            priorities._grow(B)
            self.idx = priorities.idx                         # the draw's own row: what set() names
        self.priorities = priorities
        self.hindsight = self._check_hindsight(hindsight, ring, B, bank.networks, priorities)
        env.policy_action                                     # (allocated here, not inside a capture)
        learners._grow(B)

    def _act(self, s):
        from . import _bank_capi
        if self.actor is not None:
            return self._act_fast(s)
        env = self.env
        _bank_capi.check(env._policy_launch(self.bank, 0.0, 0, env._tick_dev.data_ptr(), s), "aquabank_act_f32")

    def _queue(self):
        """the eight stages on torch's current stream, every draw keyed by the device tick base or the update counters"""
        env, ring = self.env, self.ring
        action, tb = env.policy_action, env._tick_dev
        s = env._stream()
        self._act(s)
        ring.before_step(action)
        _capi.check(env._step_launch(action.data_ptr(), _capi.ACT_U8, 0, 0, tb.data_ptr(), env.reward.data_ptr(),
                                     env.term.data_ptr(), env.done_bits.data_ptr(), s), "aqua_step_f32")
        ring.after_step()
        per = self.priorities
        if per is not None:
            per.insert()                                      # the batch just closed, with the largest priority so far
        self.tracker.after_step()
        if self.segments is not None:
            self.segments.account()
        if self.selector is not None:
            self.selector.select()
        # the uniform draw and the bank's update, or the descent of the sum trees and the update with its weights
        draw = self.learners.draw(ring, self.batch_size, out=self.idx) if per is None else per.draw(self.batch_size, out=self.idx)
        update = self.learners.update if per is None else per.update
        if self.hindsight is not None:
            her = self.hindsight
            her.relabel(draw, self.learners)                  # keyed by the learners' t, which the update below advances
            update(her.view, self.batch_size, her.idx)
        elif self.nstep is None:
            update(self.view, self.batch_size, draw)
        else:
            nstep = self.nstep
            nstep.fold(draw, hyper=self.learners.hyper)       # the table as the selector left it -> gamma^n, on the device
            update(nstep.view, self.batch_size, nstep.idx, hyper=nstep.hyper)
        if per is not None:
            per.set(draw)                                     # the slots of the draw, not the staged positions
        if self.actor is not None:
            self.actor.refresh()                              # every slot, behind the selector's copy and the update
        _capi.check(_capi.lib.aqua_tick_advance(tb.data_ptr(), 1, s), "aqua_tick_advance")

    def _warm_up(self):
        """DQNLoop._warm_up's rule: every kernel of the iteration runs once, on the current stream, and leaves no trace.  The
        bank writes policy_action (an output); the accounting sees a batch in which no world counts; the ring kernels and the
        bank draw run on a one-slot scratch ring; the SegmentTracker, if there is one, finds no new record; the selector, if
        there is one, runs on scratch state in which no network has finished an episode; the learner bank
        gets minibatches without a sample (documented to leave everything but loss and grad as it was, and those are put
        back); the fold, if there is one, runs on scratch rows and a scratch table with a draw without a sample; a
        PrioritizedReplay, if there is one, runs on a scratch tree and its update takes the learner bank's place; the step is
        taken on a snapshot and taken back."""
        from . import _lbank_capi
        torch, env, tracker, learners = self.torch, self.env, self.tracker, self.learners
        dev, n = env.device, env.num_envs
        rpl = self.ring._capi
        s = env._stream()
        tb = env._tick_dev
        self._act(s)
        if self.actor is not None:
            self.actor.refresh()                              # (the weights have not changed: the same bytes again)
        tracker.after_step(torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                           torch.full((n,), -1, dtype=torch.int32, device=dev))
        if self.segments is not None:
            self.segments.account()                                          # no new record: its cursor is the log's already
        if self.selector is not None:
            self.selector._warm_up()                                         # scratch state, nobody scored: nothing is copied
        header = torch.zeros(rpl.HEADER_WORDS, dtype=torch.int64, device=dev)
        rows = torch.zeros((5, 1), dtype=torch.float32, device=dev)
        f32, u8 = torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(3, dtype=torch.uint8, device=dev)
        idx = torch.full_like(self.idx, -1)
        rpl.check(rpl.lib.aquarpl_open(header.data_ptr(), rows.data_ptr(), u8[0:].data_ptr(), u8[1:].data_ptr(), 1, 1, rows.data_ptr(), 1,
                                       u8[2:].data_ptr(), rpl.ACT_U8, 1, None, 1, s), "aquarpl_open")
        rpl.check(rpl.lib.aquarpl_close(header.data_ptr(), f32.data_ptr(), rows.data_ptr(), u8[0:].data_ptr(), 1, 1, f32.data_ptr(),
                                        rows.data_ptr(), 1, u8[2:].data_ptr(), 1, s), "aquarpl_close")
        _lbank_capi.check(_lbank_capi.lib.aqualbank_draw(header.data_ptr(), u8[1:].data_ptr(), 1, 1, 1, learners.networks,
                                                         learners.t.data_ptr(), learners.seed_dev.data_ptr(), idx.data_ptr(),
                                                         self.batch_size, s), "aqualbank_draw")
        idx.fill_(-1)
        if self.nstep is not None:
            self.nstep._warm_up(with_table=True)
        if self.hindsight is not None:
            self.hindsight._warm_up(with_table=True)
        if self.priorities is not None:
            self.priorities._warm_up(self.view)                              # scratch trees; its update, without a sample
        else:
            loss = learners.loss.clone()
            grad = learners.grad.clone()
            learners.update(self.view, self.batch_size, idx)                 # no sample: nothing but loss and grad is written
            learners.loss.copy_(loss)
            learners.grad.copy_(grad)
        snap = env.snapshot()
        _capi.check(env._step_launch(env.policy_action.data_ptr(), _capi.ACT_U8, 0, 0, tb.data_ptr(), env.reward.data_ptr(),
                                     env.term.data_ptr(), env.done_bits.data_ptr(), s), "aqua_step_f32")
        env.restore(snap)
        _capi.check(_capi.lib.aqua_tick_advance(tb.data_ptr(), 0, s), "aqua_tick_advance")
        torch.cuda.current_stream(dev).synchronize()
