#!/usr/bin/env python3
"""P DQN trainings with different learning rates and discounts on ONE batch of worlds, entirely on the device: what
main/impl/dqn.py:11-13 prepares for ("to allow multiple trainings in parallel") as one captured graph.

Network p of a QNetworkBank acts in worlds [p * seg, (p + 1) * seg) (libaqua_bank.so); one batched step moves every world;
the transitions of all networks land in the one device experience ring; DQNLearnerBank (libaqua_lbank.so) draws every
network's minibatch from its own slots of that ring and updates all P networks in two launches.  The whole iteration is
trainer.PopulationLoop: eleven kernels, one graph launch from Python.

Exploration: network p explores with eps[p], a device array the graph reads and a SegmentTracker (libaqua_segments.so)
advances inside the graph: once per episode the network's worlds finish, as dqn.py:184 does.  The same launch keeps every
network's mean reward and success rate over its last 100 episodes (dqn.py:196-198) on the device.  Nothing is read back
between two prints, and a print reads P numbers of each.

--pbt selects among the networks while they train (population-based training, libaqua_pbt.so): every --pbt-every
iterations the worst --pbt-fraction of the networks that have finished --pbt-ready episodes since their last replacement
take the weights, the optimiser state and the perturbed lr and gamma of networks drawn from the best --pbt-fraction, inside
the graph: thirteen kernels.  Each print then shows every slot's current lr and gamma, the initial network it descends from
and the replacements so far.

--fast acts through FastActor(bank): the hidden layers of every network on the f16 MFMA with operands split hi / lo; one
refresh of the split weights follows the update inside the graph, one kernel more.

--host-refresh keeps the loop as it was before that library: ten kernels, eps refreshed from the host every --refresh
iterations from the tracker's log, the statistics rebuilt on the host from the log.

--n-step K learns the K-step target: one more kernel folds the draw (nstep.NStepReturns) and derives every network's
gamma^K from the learners' device table, so a gamma --pbt has just perturbed is the one the same iteration bootstraps with.

--per replaces the uniform draw by prioritised replay (priority.PrioritizedReplay, libaqua_prio.so): a sum tree per network
over its slots of the ring, importance weights in the update, the new TD errors back into the tree -- three more kernels, all
inside the graph.  --per-alpha, --per-beta0 and --per-anneal are the exponent of the priorities, the first importance exponent
and the updates over which it rises to 1.

--her relabels the goals of every network's drawn transitions in hindsight (hindsight.HindsightReplay, libaqua_her.so): one
more kernel replays a share --her-ratio of them under a goal their own world reached within the next --her-horizon steps,
keyed by the learners' device counters and keys.  Not together with --n-step or --per.

    python examples/dqn_population.py [--networks 8] [--seg 256] [--steps 3000] [--batch 64] [--obstacles] [--host-refresh]
                                      [--pbt] [--pbt-ready 100] [--pbt-fraction 0.25] [--pbt-every 1] [--fast] [--n-step 3]
                                      [--per] [--per-alpha 0.6] [--per-beta0 0.4] [--per-anneal 100000]
                                      [--her] [--her-ratio 0.8] [--her-horizon 32]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.episodes import EpisodeTracker
from aquaticgymenv_amd.lbank import DQNLearnerBank
from aquaticgymenv_amd.qbank import QNetworkBank
from aquaticgymenv_amd.replay import DeviceReplayRing
from aquaticgymenv_amd.segments import SegmentTracker
from aquaticgymenv_amd.trainer import PopulationLoop

ap = argparse.ArgumentParser()
ap.add_argument("--networks", type=int, default=8)
ap.add_argument("--seg", type=int, default=256, help="worlds per network")
ap.add_argument("--steps", type=int, default=3000)
ap.add_argument("--batch", type=int, default=64, help="samples per network and update (the reference: 64)")
ap.add_argument("--rounds", type=int, default=256, help="batched steps the ring holds (its capacity is rounds x worlds)")
ap.add_argument("--obstacles", action="store_true")
ap.add_argument("--epsilon-decay", type=float, default=10000, help="episodes of a network to reach the final epsilon")
ap.add_argument("--host-refresh", action="store_true", help="the schedule and the statistics on the host, as before the SegmentTracker")
ap.add_argument("--refresh", type=int, default=50, help="with --host-refresh: iterations between two refreshes of the epsilon array")
ap.add_argument("--pbt", action="store_true", help="select among the networks on the device (population-based training)")
ap.add_argument("--pbt-ready", type=int, default=100, help="episodes a network finishes before it can be replaced (again)")
ap.add_argument("--pbt-fraction", type=float, default=0.25, help="the quantile that is replaced, and the one parents are drawn from")
ap.add_argument("--pbt-every", type=int, default=1, help="iterations between two selections")
ap.add_argument("--fast", action="store_true", help="act on the f16 MFMA, operands split hi / lo (FastActor over the bank)")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--n-step", type=int, default=1, help="the window of the multi-step target (1: the reference's one-step target)")
ap.add_argument("--per", action="store_true", help="prioritised experience replay on the device (PrioritizedReplay)")
ap.add_argument("--per-alpha", type=float, default=0.6, help="with --per: the exponent of the priorities (0: uniform)")
ap.add_argument("--per-beta0", type=float, default=0.4, help="with --per: the importance exponent of the first update")
ap.add_argument("--per-anneal", type=int, default=100000, help="with --per: updates over which the importance exponent rises to 1")
ap.add_argument("--her", action="store_true", help="hindsight experience replay on the device (HindsightReplay)")
ap.add_argument("--her-ratio", type=float, default=0.8, help="with --her: the share of the eligible samples that is relabelled")
ap.add_argument("--her-horizon", type=int, default=32, help="with --her: how many steps ahead a goal may lie")
args = ap.parse_args()
if args.her and (args.per or args.n_step != 1):
    ap.error("--her relabels one stored step under a uniform draw: it does not go with --n-step or --per")
if args.pbt and args.host_refresh:
    ap.error("--pbt judges the networks by the SegmentTracker's statistics: it does not go with --host-refresh")

EPS_INIT, EPS_FINAL, TAU = 1.0, 0.05, 0.005                   # default_hyperparam of dqn.py
P, seg = args.networks, args.seg
worlds = P * seg
# the sweep: learning rates a factor 10 around dqn.py's 1e-3, discounts between 0.9 and 0.99
lrs = [1e-3 * 10.0 ** ((p % 4 - 1.5) / 3.0) for p in range(P)]
gammas = [0.9 + 0.09 * (p // 4) / max((P - 1) // 4, 1) for p in range(P)]

rng = np.random.RandomState(args.seed)
networks = []
for p in range(P):                                             # Keras' default: Glorot-uniform kernels, zero biases
    layers = []
    for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        layers.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))
    networks.append(layers)
bank = QNetworkBank(networks, seg, "cuda")
learners = DQNLearnerBank(bank, gamma=gammas, tau=TAU, lr=lrs, strategy="double_ref", seed=args.seed)

env = BatchedAqua(worlds, obstacles=args.obstacles, seed=args.seed, auto_reset="next_step", normalized_obs=True)
env.reset()
ring = DeviceReplayRing(env, capacity=args.rounds * worlds)   # a multiple of the batch: a slot belongs to one world
tracker = EpisodeTracker(env)
segments = None
if args.host_refresh:
    eps = torch.full((P,), EPS_INIT, dtype=torch.float32, device=bank.device)
else:
    segments = SegmentTracker(tracker, seg, P, window=100, epsilon=(EPS_INIT, EPS_FINAL, args.epsilon_decay))
    eps = segments.epsilon
bank.epsilon = eps
selector = None
if args.pbt:
    from aquaticgymenv_amd.pbt import PopulationSelector
    selector = PopulationSelector(learners, segments, score="mean_return", fraction=args.pbt_fraction, ready=args.pbt_ready,
                                  every=args.pbt_every, seed=args.seed)
actor = None
if args.fast:
    from aquaticgymenv_amd.fastpolicy import FastActor
    actor = FastActor(bank)
priorities = None
if args.per:
    from aquaticgymenv_amd.priority import PrioritizedReplay
    priorities = PrioritizedReplay(ring, learners, alpha=args.per_alpha, beta0=args.per_beta0, anneal=args.per_anneal)
hindsight = None
if args.her:
    from aquaticgymenv_amd.hindsight import HindsightReplay
    hindsight = HindsightReplay(ring, args.batch, networks=P, horizon=args.her_horizon, ratio=args.her_ratio)
graph = PopulationLoop(env, bank, learners, ring, tracker, args.batch, segments=segments, selector=selector, actor=actor, n_step=args.n_step,
                       priorities=priorities, hindsight=hindsight).capture()
decay = (EPS_FINAL / EPS_INIT) ** (1.0 / args.epsilon_decay)  # dqn.py:139-140
episodes, seen = np.zeros(P, dtype=np.int64), 0               # --host-refresh: finished episodes per network, and in all
for step in range(1, args.steps + 1):
    graph.launch()                                             # act, record, step, record, account, [segments,] draw, update, tick
    if args.host_refresh and step % args.refresh == 0:         # host reads: the new records, then P floats back to the device
        total = tracker.counts()["episodes"]
        new = tracker.last(total - seen)                       # (at most the log's capacity of them)
        episodes += np.bincount(new["world"] // seg, minlength=P)[:P]
        seen = total
        eps.copy_(torch.from_numpy(np.maximum(EPS_FINAL, EPS_INIT * decay ** episodes).astype(np.float32)))
    if step % 100 == 0:
        loss = learners.loss.cpu().numpy()
        print("step %6d  episodes %7d  ring %d" % (step, tracker.counts()["episodes"], ring.filled()))
        if segments is not None:                               # P numbers each, as the device published them
            done = [r["episodes"] for r in segments.counts()["segments"]]
            last = [min(d, segments.window) for d in done]
            reward, success = segments.mean_return.cpu().numpy(), segments.success_rate.cpu().numpy()
        else:                                                  # the log read back and sorted out by owner on the host
            log = tracker.last(tracker.capacity)
            owner = log["world"] // seg
            mine = [np.nonzero(owner == p)[0][-100:] for p in range(P)]
            last = [m.size for m in mine]
            reward = [float(log["ret"][m].sum()) / max(m.size, 1) for m in mine]
            success = [float((log["code"][m] == 3).sum()) / max(m.size, 1) for m in mine]
        now = eps.cpu().numpy()
        if selector is not None:                               # a host read: the counters, the lineage, and the table selection rewrites
            report = selector.report()                         # (calls learners.sync_hyper(): hyper_of() is current again)
            lrs, gammas = ([learners.hyper_of(p)[key] for p in range(P)] for key in ("lr", "gamma"))
            print("    selections %d  replaced %d (%d by the last)  descend from %s" %
                  (report["calls"], report["replaced"], report["last"], report["origin"].tolist()))
        for p in range(P):
            print("    network %3d  lr %.2e  gamma %.3f  epsilon %.3f  last %3d episodes: reward %8.2f  success %3.0f %%  loss %10.4f" %
                  (p, lrs[p], gammas[p], float(now[p]), last[p], float(reward[p]), 100.0 * float(success[p]), float(loss[p])))
for p in range(P):
    learners.weights(p)                                        # bank.layers[p] now holds the trained network p
