#!/usr/bin/env python3
"""The reference's DQN training loop (main/impl/dqn.py:139-184) on a batch of worlds, entirely on the device: the
epsilon-greedy Q-network picks the actions (libaqua_policy.so), one batched step moves every world, the transitions land in
the device experience ring, and DQNLearner (libaqua_learner.so) performs the update -- TD target, gradient, Adam, soft
target update -- and re-packs the acting network's weights in place.

One batched step here is N steps of the reference, and one update of --batch samples follows it.  The episodes are kept by
an EpisodeTracker (libaqua_episodes.so) on the device: return and length per world, the log of finished episodes, and
epsilon, which decays once per finished episode as dqn.py:184 does and is read by the exploration pass where it lives.
Every 100 steps the line of dqn.py:194-200 is printed from the tracker -- mean return, mean length and success rate of the
last 100 episodes, epsilon; that print is the only host read of the loop.

By default the whole iteration -- act, explore, record, step, record, account, draw, update -- is ONE captured graph
(trainer.DQNLoop over a DeviceReplayRing, whose cursor and size live on the device): one launch from Python per iteration
instead of about sixteen.  --eager keeps the loop written out call by call with ReplayRing; both compute the same bits.

--fast acts through a FastActor over the trained network (the hidden layers on the f16 MFMA, operands split hi / lo); its
split copy of the weights is refreshed after every update, inside the graph: one kernel more.

--n-step K learns the K-step target: one more kernel in the graph folds the K transitions that follow every drawn one into a
staged minibatch (nstep.NStepReturns), and the update bootstraps with gamma^K.  The ring then holds whole batched steps.

--her relabels the goals of the drawn transitions in hindsight (hindsight.HindsightReplay, libaqua_her.so): one more kernel in
the graph replays a share --her-ratio of them under a goal their own world reached within the next --her-horizon steps, with
the reward recomputed exactly.  The ring then holds whole batched steps.  Not together with --n-step or --eager.

    python examples/dqn_train.py [--envs 1024] [--steps 3000] [--batch 256] [--obstacles] [--eager] [--fast] [--n-step 3]
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
from aquaticgymenv_amd.learner import DQNLearner
from aquaticgymenv_amd.qpolicy import QNetwork
from aquaticgymenv_amd.replay import DeviceReplayRing, ReplayRing
from aquaticgymenv_amd.trainer import DQNLoop

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1024)
ap.add_argument("--steps", type=int, default=3000)
ap.add_argument("--batch", type=int, default=256, help="samples per update (the reference: 64, one world)")
ap.add_argument("--buffer", type=int, default=1 << 20, help="ring capacity in transitions")
ap.add_argument("--obstacles", action="store_true")
ap.add_argument("--epsilon-decay", type=float, default=10000, help="a factor, or the number of episodes to reach the final epsilon")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--loss", choices=("mse", "reference"), default="mse",
                help="mse: the mean squared TD error; reference: the broadcast loss main/impl/dqn.py:243-247 executes")
ap.add_argument("--eager", action="store_true", help="issue every launch of the iteration from Python (ReplayRing) instead of replaying one graph")
ap.add_argument("--fast", action="store_true", help="act on the f16 MFMA, operands split hi / lo (FastActor, refreshed after every update)")
ap.add_argument("--n-step", type=int, default=1, help="the window of the multi-step target (1: the reference's one-step target)")
ap.add_argument("--her", action="store_true", help="hindsight experience replay on the device (HindsightReplay)")
ap.add_argument("--her-ratio", type=float, default=0.8, help="with --her: the share of the eligible samples that is relabelled")
ap.add_argument("--her-horizon", type=int, default=32, help="with --her: how many steps ahead a goal may lie")
args = ap.parse_args()
if args.n_step != 1 and args.eager:
    ap.error("--n-step folds the device ring: it goes with the graph, not with --eager")
if args.her and (args.eager or args.n_step != 1):
    ap.error("--her relabels from the device ring, one step at a time: it goes with the graph, and not with --n-step")

# default_hyperparam of dqn.py
EPS_INIT, EPS_FINAL, GAMMA, TAU = 1.0, 0.05, 0.98, 0.005

rng = np.random.RandomState(args.seed)
layers = []
for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):          # Keras' default: Glorot-uniform kernels, zero biases
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    layers.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))
qnet = QNetwork(layers, "cuda")
learner = DQNLearner(qnet, gamma=GAMMA, tau=TAU, lr=1e-3, strategy="double_ref", seed=args.seed, loss=args.loss)

env = BatchedAqua(args.envs, obstacles=args.obstacles, seed=args.seed, auto_reset="next_step", normalized_obs=True)
env.reset()
capacity = max(args.buffer, args.envs)
if args.n_step != 1 or args.her:
    capacity -= capacity % args.envs                           # whole batched steps: a world's next step is one batch further
ring = (ReplayRing if args.eager else DeviceReplayRing)(env, capacity=capacity)
tracker = EpisodeTracker(env, epsilon=(EPS_INIT, EPS_FINAL, args.epsilon_decay))     # decay >= 1: episodes to reach EPS_FINAL
actor = None
if args.fast:
    from aquaticgymenv_amd.fastpolicy import FastActor
    actor = FastActor(qnet)
hindsight = None
if args.her:
    from aquaticgymenv_amd.hindsight import HindsightReplay
    hindsight = HindsightReplay(ring, args.batch, horizon=args.her_horizon, ratio=args.her_ratio)
graph = None if args.eager else DQNLoop(env, qnet, learner, ring, tracker, args.batch, actor=actor, n_step=args.n_step,
                                        hindsight=hindsight).capture()
for step in range(1, args.steps + 1):
    if graph is not None:
        graph.launch()                                         # the nine stages below and the tick advance, as one graph
    else:
        # env.step(policy=qnet, epsilon=...) in three calls: greedy actions, the exploring draws under the device epsilon, and
        # the step, so that the ring sees the action before the step
        action = (actor or qnet).act(env, epsilon=0.0, out=env.policy_action)
        tracker.explore(env.policy_action)
        ring.before_step(env.policy_action)
        obs, reward, term = env.step(action)
        ring.after_step()
        tracker.after_step()                                   # returns, lengths, the log, epsilon: all on the device
        learner.update(ring, args.batch)                       # minibatch drawn on the device; qnet acts with the new weights
        if actor is not None:
            actor.refresh()                                    # ... and the fast actor after its re-split
    if step % 100 == 0:                                        # the only host reads of the loop
        c, last = tracker.counts(), tracker.last(100)
        k = max(len(last["ret"]), 1)
        print("step %6d  episodes %7d  mean_last_100: reward %8.2f  steps %6.1f  success %3.0f %%  loss %10.4f  epsilon %.3f  ring %d" %
              (step, c["episodes"], float(last["ret"].sum()) / k, float(last["len"].sum()) / k,
               100.0 * float((last["code"] == 3).sum()) / k, float(learner.loss), float(tracker.epsilon), ring.size if args.eager else ring.filled()))
learner.weights()                                              # qnet.layers now holds the trained network
