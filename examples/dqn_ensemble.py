#!/usr/bin/env python3
"""Train a small population of DQN networks on the device, then let them act TOGETHER (ensemble.QEnsemble, libaqua_ens.so).

1. trainer.PopulationLoop trains P networks on one batch of P x seg worlds, as examples/dqn_population.py does.
2. Every member alone: episodes.evaluate(env, bank) on a fresh auto_reset=False batch of P segments of --eval worlds, the
   bank's network p on segment p (the segments are different worlds of one seeded batch).
3. The ensemble, in both modes: evaluate(env, QEnsemble(bank, mode=...)) on a fresh batch of --eval worlds with the same seed.
   One launch per step evaluates all P networks on every world and acts on their mean Q / their majority vote.

It prints the success rates.  Whatever it prints is the observation of ONE seed and one short training: it shows how the
pieces go together, it is no evidence that an ensemble is better (or worse) than its best member.

    python examples/dqn_ensemble.py [--networks 4] [--seg 256] [--steps 2000] [--batch 64] [--eval 1024] [--obstacles] [--seed 0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.ensemble import QEnsemble
from aquaticgymenv_amd.episodes import EpisodeTracker, evaluate
from aquaticgymenv_amd.lbank import DQNLearnerBank
from aquaticgymenv_amd.qbank import QNetworkBank
from aquaticgymenv_amd.replay import DeviceReplayRing
from aquaticgymenv_amd.segments import SegmentTracker
from aquaticgymenv_amd.trainer import PopulationLoop

ap = argparse.ArgumentParser()
ap.add_argument("--networks", type=int, default=4)
ap.add_argument("--seg", type=int, default=256, help="worlds per network while training")
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--batch", type=int, default=64, help="samples per network and update (the reference: 64)")
ap.add_argument("--rounds", type=int, default=256, help="batched steps the ring holds")
ap.add_argument("--eval", type=int, default=1024, help="worlds per evaluation (per member, and for the ensemble)")
ap.add_argument("--epsilon-decay", type=float, default=2000, help="episodes of a network to reach the final epsilon")
ap.add_argument("--obstacles", action="store_true")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

P, seg = args.networks, args.seg
worlds = P * seg
rng = np.random.RandomState(args.seed)
networks = []
for p in range(P):                                             # Keras' default: Glorot-uniform kernels, zero biases
    layers = []
    for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        layers.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))
    networks.append(layers)

# ---- 1. train
bank = QNetworkBank(networks, seg, "cuda")
learners = DQNLearnerBank(bank, gamma=0.98, tau=0.005, lr=1e-3, strategy="double_ref", seed=args.seed)
env = BatchedAqua(worlds, obstacles=args.obstacles, seed=args.seed, auto_reset="next_step", normalized_obs=True)
env.reset()
ring = DeviceReplayRing(env, capacity=args.rounds * worlds)
tracker = EpisodeTracker(env)
segments = SegmentTracker(tracker, seg, P, window=100, epsilon=(1.0, 0.05, args.epsilon_decay))
bank.epsilon = segments.epsilon
graph = PopulationLoop(env, bank, learners, ring, tracker, args.batch, segments=segments).capture()
for step in range(1, args.steps + 1):
    graph.launch()
    if step % 500 == 0:
        print("step %6d  episodes %7d  success over the last 100 episodes per network: %s" %
              (step, tracker.counts()["episodes"], ["%.2f" % v for v in segments.success_rate.cpu().numpy()]))
torch.cuda.synchronize()
bank.epsilon = None                                            # evaluation is greedy

# ---- 2. every member alone: network p on segment p of one batch
n = args.eval
alone = QNetworkBank([bank.view(p).weights() for p in range(P)], n, "cuda")
env = BatchedAqua(P * n, obstacles=args.obstacles, seed=args.seed + 1, auto_reset=False)
env.reset()
rates = alone.split(evaluate(env, alone)["Success"]).mean(axis=1)
for p in range(P):
    print("network %3d alone      success %5.1f %%  (%d episodes)" % (p, 100.0 * rates[p], n))

# ---- 3. the ensemble: all P networks on every world, one launch per step
for mode in ("mean", "vote"):
    env = BatchedAqua(n, obstacles=args.obstacles, seed=args.seed + 1, auto_reset=False)
    env.reset()
    rate = evaluate(env, QEnsemble(alone, mode=mode))["Success"].mean()
    print("ensemble of %d, %-5s  success %5.1f %%  (%d episodes)" % (P, mode, 100.0 * rate, n))
print("one seed, one short training: an observation, not a comparison")
