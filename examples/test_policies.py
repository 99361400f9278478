#!/usr/bin/env python3
"""The reference's test protocol (main/plotting/dqn_test_plotter.py::run_tests: every policy of tests_config, n_tests
episodes each, success rate and mean reward per label) for BOTH shipped policies in ONE batch: the first half of the
worlds has no obstacles and acts with the "No obstacles" policy, the second half has the obstacle preset (per-world
tables) and acts with the "With obstacles" policy.  One QNetworkBank, one episodes.evaluate(): every step is one policy
launch for both networks and one step launch for both kinds of world.

    python examples/test_policies.py [episodes per policy = 1000] [seed = 9001]

The weights and the published per-episode results come from tests/golden/dqn_policies.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS = (("No obstacles", "no_obs", False), ("With obstacles", "with_obs", True))


def main():
    # imported here: the file carries the reference's name, test_*.py, and a bare `pytest` at the repository's root
    # imports it while collecting; that must not load the HIP libraries (the suite is `pytest tests`)
    sys.path.insert(0, ROOT)
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import evaluate
    from aquaticgymenv_amd.qbank import QNetworkBank
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 9001
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    bank = QNetworkBank([[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for _, tag, _ in LABELS], n, "cuda:0")
    tables = np.zeros((len(LABELS) * n, presets.DEFAULT5.shape[0], 5), dtype=np.float64)
    for p, (_, _, obstacles) in enumerate(LABELS):
        if obstacles:
            tables[p * n:(p + 1) * n] = presets.DEFAULT5
        else:
            tables[p * n:(p + 1) * n, :, 2] = -1.0          # kind < 0: an absent row
    env = BatchedAqua(len(LABELS) * n, obstacles=tables, seed=seed, auto_reset=False, device="cuda:0")
    env.reset()
    result = evaluate(env, bank)
    success, reward = bank.split(result["Success"]), bank.split(result["Reward"])
    for p, (label, tag, _) in enumerate(LABELS):
        print("%-15s %d episodes: success %5.1f %% (published %.1f %%), mean reward %8.2f (published %.2f)"
              % (label, n, 100.0 * success[p].mean(), 100.0 * z[tag + "_published_success"].mean(), reward[p].mean(),
                 z[tag + "_published_reward"].mean()))


if __name__ == "__main__":
    main()
