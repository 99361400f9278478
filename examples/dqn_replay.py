#!/usr/bin/env python3
"""Replay one of the reference's trained DQN policies (5-64-64-3 MLP, weights committed as a test fixture, read from
the reference's SavedModel without TensorFlow by aquaticgymenv_amd.tf_import, evaluated by aquaticgymenv_amd.qpolicy.QNetwork
-- tf_import.GreedyQPolicy is the same network as torch GEMMs) on a batch of worlds: first one episode per world, the way
Policy.test / TestPlotter.run_tests of the reference evaluate a policy (aquaticgymenv_amd.episodes.evaluate), then 500 steps
with restarts, recording the transitions into the device-side experience ring the way main/impl/dqn.py:174 appends them to
its deque.

--fast acts through FastActor (aquaticgymenv_amd.fastpolicy): the hidden layers on the f16 MFMA with operands split hi / lo,
the same policy at float32-like accuracy in about 0.6 of the float32 kernel's time.

    python examples/dqn_replay.py [--envs 16384] [--obstacles] [--fast]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.episodes import evaluate
from aquaticgymenv_amd.replay import ReplayRing
from aquaticgymenv_amd.qpolicy import QNetwork

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=16384)
ap.add_argument("--obstacles", action="store_true", help="the policy trained with the default five obstacles")
ap.add_argument("--fast", action="store_true", help="act on the f16 MFMA, operands split hi / lo (FastActor)")
args = ap.parse_args()

z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
tag = "with_obs" if args.obstacles else "no_obs"
qnet = QNetwork([(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)], "cuda")
if args.fast:
    from aquaticgymenv_amd.fastpolicy import FastActor
    qnet = FastActor(qnet)                                 # a policy wherever the QNetwork is one; its weights are fixed here

# one episode per world, no restarts: the protocol of the published figures
runs = BatchedAqua(args.envs, obstacles=args.obstacles, seed=2, auto_reset=False)
runs.reset()
result = evaluate(runs, qnet)
print("%d runs, %d finished: %.1f %% reached the goal (published: %.1f %%), mean reward %.2f (published %.2f), mean steps %.1f" %
      (args.envs, int((result["Code"] != 0).sum()), 100.0 * float(result["Success"].mean()),
       100.0 * float(z["%s_published_success" % tag].mean()), float(result["Reward"].mean()),
       float(z["%s_published_reward" % tag].mean()), float(result["Steps"].mean())))

env = BatchedAqua(args.envs, obstacles=args.obstacles, seed=2, auto_reset="next_step", normalized_obs=True)
env.reset()
ring = ReplayRing(env, capacity=64 * args.envs)
for step in range(500):
    action = qnet.act(env, out=env.policy_action)          # argmax_a Q(s, a): one launch of our own kernel (epsilon=... explores)
    ring.before_step(env.policy_action)
    obs, reward, term = env.step(action)
    ring.after_step()
s, a, r, s2, done = ring.sample(256)
q_next = qnet.q_values(ring.s2, ring.size)                 # Q(s', .) of the whole ring for TD targets (dqn.py:262-292): [3][size]
print("ring holds %d transitions; a sampled minibatch: s %s a %s r %s s' %s done %s" %
      (ring.size, tuple(s.shape), tuple(a.shape), tuple(r.shape), tuple(s2.shape), tuple(done.shape)))
print("max_a Q(s', a) over the ring: mean %.3f" % float(q_next.max(dim=0).values.mean()))
