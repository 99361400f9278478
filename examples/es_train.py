#!/usr/bin/env python3
"""Train the Q-network's weights by evolution strategies on the device (evolution.EvolutionStrategy, libaqua_evo.so): no
replay ring, no TD target, no backward pass.

A bank of --networks networks holds the antithetic perturbations theta +- sigma eps of one centre; with an odd number the last
slot flies the centre itself.  A generation is es.generation(env): ask() fills the bank, every network flies one episode in each
of its --seg worlds of an auto_reset=False batch on the obstacle-free discrete env, fitness() scores the networks from the
episode log and tell() steps the centre along the rank differences.  Per generation it prints the mean and the best fitness of
the population and the centre's own (the last slot).  At the end the centre alone is evaluated on fresh worlds: write_centre()
hands it to a plain QNetwork.

Whatever it prints is the observation of ONE seed: it shows how the pieces go together, it is no evidence of how fast evolution
strategies learn this task, beside examples/dqn_train.py or at all.

    python examples/es_train.py [--networks 65] [--seg 64] [--generations 50] [--sigma 0.05] [--lr 0.01] [--score success_rate]
                                [--eval 4096] [--seed 0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from aquaticgymenv_amd import EvolutionStrategy
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.episodes import evaluate
from aquaticgymenv_amd.qbank import QNetworkBank
from aquaticgymenv_amd.qpolicy import QNetwork

ap = argparse.ArgumentParser()
ap.add_argument("--networks", type=int, default=65, help="P: an odd number keeps the centre in the last slot")
ap.add_argument("--seg", type=int, default=64, help="worlds (episodes) per network and generation")
ap.add_argument("--generations", type=int, default=50)
ap.add_argument("--sigma", type=float, default=0.05)
ap.add_argument("--lr", type=float, default=0.01)
ap.add_argument("--optimizer", default="adam", choices=("adam", "sgd"))
ap.add_argument("--weight-decay", type=float, default=0.0)
ap.add_argument("--score", default="mean_return", choices=("mean_return", "success_rate"))
ap.add_argument("--eval", type=int, default=4096, help="worlds of the centre's final evaluation")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

P, seg = args.networks, args.seg
rng = np.random.RandomState(args.seed)
centre = []
for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):               # Keras' default: Glorot-uniform kernels, zero biases
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    centre.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))

bank = QNetworkBank([centre] * P, seg, "cuda")
es = EvolutionStrategy(bank, centre=centre, sigma=args.sigma, lr=args.lr, seed=args.seed, optimizer=args.optimizer,
                       weight_decay=args.weight_decay, score=args.score)
env = BatchedAqua(P * seg, obstacles=False, seed=args.seed, auto_reset=False)      # evaluate() resets it every generation
for g in range(args.generations):
    fitness = es.generation(env).cpu().numpy()
    flown = fitness[:2 * (P // 2)]
    own = "%9.3f" % fitness[-1] if P % 2 else "   (none)"
    print("generation %4d  %s: mean %9.3f  best %9.3f (slot %d)  centre %s" %
          (g, args.score, flown.mean(), flown.max(), es.report()["best"], own))

# the centre alone, on fresh worlds
qnet = es.write_centre(QNetwork(centre, "cuda"))
env = BatchedAqua(args.eval, obstacles=False, seed=args.seed + 1, auto_reset=False)
env.reset()
result = evaluate(env, qnet)
print("the centre after %d generations: success %5.1f %%, mean return %.3f  (%d fresh episodes)" %
      (args.generations, 100.0 * result["Success"].mean(), result["Reward"].mean(), args.eval))
print("one seed: an observation, not a measurement of how fast evolution strategies learn this task")
