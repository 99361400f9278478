#!/usr/bin/env python3
"""Times one DQN training iteration three ways, in microseconds of wall clock per iteration:

  eager   the loop of examples/dqn_train.py --eager: ReplayRing (cursor and size on the host), learner.update(ring, B)
          drawing for itself -- about sixteen launches issued from Python
  step    trainer.DQNLoop.step(): the same nine stages on a DeviceReplayRing, eleven launches issued from Python
  graph   trainer.DQNLoop.capture().launch(): the same eleven kernels as one captured graph

Per batch size (default 1 024, 16 384 and 262 144 worlds, minibatch 256): every variant has its own env, network, learner,
ring and tracker from the same seeds, is warmed up, and is then timed in windows of --iters iterations between a
synchronise and a synchronise with a HOST clock -- the eager loop is bound by the host, so wall clock is the honest clock
here.  The variants alternate inside one repeat; the median and the spread (min .. max) over --repeats windows are printed
as one JSON line per batch size.  Needs a GPU: there is nothing to time without one.

    python tools/train_bench.py [--envs 1024 16384 262144] [--batch 256] [--iters 500] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 16384, 262144])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--buffer", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_bench.py needs a GPU")
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing, ReplayRing
    from aquaticgymenv_amd.trainer import DQNLoop

    def parts(n, device_ring):
        rng = np.random.RandomState(0)
        layers = []
        for fan_in, fan_out in ((5, 64), (64, 64), (64, 3)):
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            layers.append((rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), np.zeros(fan_out, dtype=np.float32)))
        qnet = QNetwork(layers, "cuda")
        learner = DQNLearner(qnet, gamma=0.98, tau=0.005, lr=1e-3, strategy="double_ref", seed=0)
        env = BatchedAqua(n, obstacles=True, seed=0, auto_reset="next_step", normalized_obs=True)
        env.reset()
        ring = (DeviceReplayRing if device_ring else ReplayRing)(env, capacity=max(args.buffer, n))
        tracker = EpisodeTracker(env, epsilon=(1.0, 0.05, 10000))
        return env, qnet, learner, ring, tracker

    lines = []
    for n in args.envs:
        env, qnet, learner, ring, tracker = parts(n, False)

        def eager():
            action = qnet.act(env, epsilon=0.0, out=env.policy_action)
            tracker.explore(env.policy_action)
            ring.before_step(env.policy_action)
            env.step(action)
            ring.after_step()
            tracker.after_step()
            learner.update(ring, args.batch)

        loop_step = DQNLoop(*parts(n, True), batch_size=args.batch)
        loop_graph = DQNLoop(*parts(n, True), batch_size=args.batch)
        graph = loop_graph.capture()
        variants = {"eager": eager, "step": loop_step.step, "graph": graph.launch}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize()
                times[name].append(1e6 * (time.perf_counter() - t0) / args.iters)          # us per iteration
        same = all(torch.equal(x, y) for x, y in ((learner.theta, loop_step.learner.theta), (learner.theta, loop_graph.learner.theta),
                                                  (env.state, loop_graph.env.state), (ring.ok, loop_graph.ring.ok)))
        row = {"envs": n, "batch": args.batch, "iters": args.iters, "repeats": args.repeats, "clock": "host wall clock, synchronised",
               "updates": int(learner.t[0]), "same_bits": bool(same)}
        for name, ts in times.items():
            ts = sorted(ts)
            row[name + "_us"] = {"median": round(ts[len(ts) // 2], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2)}
        row["graph_speedup_over_eager"] = round(row["eager_us"]["median"] / row["graph_us"]["median"], 2)
        lines.append(json.dumps(row, sort_keys=True))
        print(lines[-1], flush=True)
        graph.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
