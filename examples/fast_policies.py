#!/usr/bin/env python3
"""examples/test_policies.py on the fast acting path: the reference's test protocol (main/plotting/dqn_test_plotter.py::
run_tests) for BOTH shipped policies in ONE batch, acted by FastActor(bank) -- both networks of the QNetworkBank on the f16
MFMA with operands split hi / lo (aquaticgymenv_amd/fastpolicy.py) -- and, with --compare, by the float32
bank on a second batch of the same seed, side by side.  The first half of the worlds has no obstacles and acts with the "No
obstacles" policy, the second half has the obstacle preset and acts with the "With obstacles" policy; every step is one
policy launch for both networks and one step launch for both kinds of world.

    python examples/fast_policies.py [--episodes 1000] [--seed 9001] [--compare]

The weights and the published per-episode results come from tests/golden/dqn_policies.npz."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aquaticgymenv_amd import presets
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.episodes import evaluate
from aquaticgymenv_amd.fastpolicy import FastActor
from aquaticgymenv_amd.qbank import QNetworkBank

LABELS = (("No obstacles", "no_obs", False), ("With obstacles", "with_obs", True))

ap = argparse.ArgumentParser()
ap.add_argument("--episodes", type=int, default=1000, help="episodes per policy")
ap.add_argument("--seed", type=int, default=9001)
ap.add_argument("--compare", action="store_true", help="also run the float32 bank on a batch of the same seed")
args = ap.parse_args()

n = args.episodes
z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
bank = QNetworkBank([[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for _, tag, _ in LABELS], n, "cuda:0")
fast = FastActor(bank)                                     # segments and split() are the bank's; the weights are fixed here
tables = np.zeros((len(LABELS) * n, presets.DEFAULT5.shape[0], 5), dtype=np.float64)
for p, (_, _, obstacles) in enumerate(LABELS):
    if obstacles:
        tables[p * n:(p + 1) * n] = presets.DEFAULT5
    else:
        tables[p * n:(p + 1) * n, :, 2] = -1.0             # kind < 0: an absent row

for name, policy in (("fast", fast), ("float32", bank))[:2 if args.compare else 1]:
    env = BatchedAqua(len(LABELS) * n, obstacles=tables, seed=args.seed, auto_reset=False, device="cuda:0")
    env.reset()
    result = evaluate(env, policy)
    success, reward = fast.split(result["Success"]), fast.split(result["Reward"])
    for p, (label, tag, _) in enumerate(LABELS):
        print("%-8s %-15s %d episodes: success %5.1f %% (published %.1f %%), mean reward %8.2f (published %.2f)"
              % (name, label, n, 100.0 * success[p].mean(), 100.0 * z[tag + "_published_success"].mean(), reward[p].mean(),
                 z[tag + "_published_reward"].mean()))
