#!/usr/bin/env python3
"""The reference's DQN training loop (main/impl/dqn.py:139-184) on a batch of worlds, entirely on the device: the
epsilon-greedy Q-network picks the actions (libaqua_policy.so), one batched step moves every world, the transitions land in
the device experience ring, and DQNLearner (libaqua_learner.so) performs the update -- TD target, gradient, Adam, soft
target update -- and re-packs the acting network's weights in place.

One batched step here is N steps of the reference, and one update of --batch samples follows it; epsilon decays per
finished episode as dqn.py:184 does.  The success rate of the episodes finished in every 100 steps is printed.

    python examples/dqn_train.py [--envs 1024] [--steps 3000] [--batch 256] [--obstacles]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.learner import DQNLearner
from aquaticgymenv_amd.qpolicy import QNetwork
from aquaticgymenv_amd.replay import ReplayRing

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--steps", type=int, default=3000)
ap.add_argument("--batch", type=int, default=256, help="samples per update (the reference: 64, one world)")
ap.add_argument("--buffer", type=int, default=1 << 20, help="ring capacity in transitions")
ap.add_argument("--obstacles", action="store_true")
ap.add_argument("--epsilon-decay", type=float, default=10000, help="a factor, or the number of episodes to reach the final epsilon")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

# default_hyperparam of dqn.py
EPS_INIT, EPS_FINAL, GAMMA, TAU = 1.0, 0.05, 0.98, 0.005
decay = args.epsilon_decay if args.epsilon_decay < 1 else (EPS_FINAL / EPS_INIT) ** (1.0 / args.epsilon_decay)

rng = np.random.RandomState(args.seed)
layers = []
for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):          # Keras' default: Glorot-uniform kernels, zero biases
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    layers.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))
qnet = QNetwork(layers, "cuda")
learner = DQNLearner(qnet, gamma=GAMMA, tau=TAU, lr=1e-3, strategy="double_ref", seed=args.seed)

env = BatchedAqua(args.envs, obstacles=args.obstacles, seed=args.seed, auto_reset="next_step", normalized_obs=True)
env.reset()
ring = ReplayRing(env, capacity=max(args.buffer, args.envs))
epsilon = EPS_INIT
finished = torch.zeros((), dtype=torch.int64, device=env.device)
succeeded = torch.zeros((), dtype=torch.int64, device=env.device)
for step in range(1, args.steps + 1):
    # env.step(policy=qnet, epsilon=...) in two calls, so that the ring sees the action before the step
    action = qnet.act(env, epsilon=epsilon, out=env.policy_action)
    ring.before_step(env.policy_action)
    obs, reward, term = env.step(action)
    ring.after_step()
    learner.update(ring, args.batch)                           # minibatch drawn on the device; qnet acts with the new weights
    finished += (term != 0).sum()
    succeeded += (term == 3).sum()
    if step % 100 == 0:                                        # the only host reads of the loop
        n, ok = int(finished), int(succeeded)
        epsilon = max(epsilon * decay ** n, EPS_FINAL)         # dqn.py:184, once per finished episode
        print("step %6d  episodes %6d  success %5.1f %%  loss %10.4f  epsilon %.3f  ring %d" %
              (step, n, 100.0 * ok / max(n, 1), float(learner.loss), epsilon, ring.size))
        finished.zero_()
        succeeded.zero_()
learner.weights()                                              # qnet.layers now holds the trained network
