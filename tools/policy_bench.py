#!/usr/bin/env python3
"""Observation -> policy -> step with the DQN's Q-network, per step, on one GPU (not bench.py: that one measures the
step kernel alone and is untouched).

    python tools/policy_bench.py [--envs 262144] [--steps 5000] [--warmup 50] [--regions 5]

262 144 worlds, presets.BENCH8, auto_reset="next_step", the `with_obs` network of tests/golden/dqn_policies.npz.  Every
leg runs --warmup steps, then --regions regions of steps/regions steps each between two HIP events; the figure is the
MEDIAN region's microseconds per step.  All legs in one process on one device, one JSON line:

  step_only            captured step reading a fixed uint8 action buffer (the floor: no policy at all)
  torch_policy         the path before the device network: normalized_obs=True, tf_import.GreedyQPolicy(obs_norm)
                       (three addmm, two relu, argmax), copy_ into the action buffer, captured step -- examples/policy_loop.py's shape
  device_policy_eager  env.step(policy=qnet): one policy launch + one step launch from Python
  device_policy_graph  env.capture_policy_step(qnet).launch(): policy kernel -> step -> tick advance as one graph
  act_only             aquapol_act_f32 alone (QNetwork.act into a fixed buffer), with its achieved TFLOP/s on
                       9 216 FLOP per world (2 x (5 x 64 + 64 x 64 + 64 x 3) multiply-adds) beside the 157.3 TF float32
                       matrix peak
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_WORLD = 2 * (5 * 64 + 64 * 64 + 64 * 3)
F32_MATRIX_PEAK_TF = 157.3


def timed(torch, step, warmup, regions, per_region):
    """-> (median us per step, [us per step of every region])"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_region):
            step()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per_region)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--regions", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("policy_bench.py measures on a GPU; none is visible")
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.tf_import import GreedyQPolicy

    dev, n = "cuda:0", args.envs
    per_region = max(1, (args.steps + args.regions - 1) // args.regions)
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    layers = [(z["with_obs_kernel%d" % i], z["with_obs_bias%d" % i]) for i in range(3)]
    qnet = QNetwork(layers, dev)
    result = {"envs": n, "steps_per_leg": per_region * args.regions, "warmup": args.warmup, "regions": args.regions,
              "obstacles": "BENCH8", "auto_reset": "next_step", "network": "with_obs 5-64-64-3", "device": torch.cuda.get_device_name(0),
              "unit": "us per step (median region)"}

    def make(**kw):
        env = BatchedAqua(n, obstacles=presets.BENCH8, seed=0, auto_reset="next_step", device=dev, **kw)
        env.reset()
        return env

    def record(name, step):
        med, all_ = timed(torch, step, args.warmup, args.regions, per_region)
        result[name] = round(med, 3)
        result[name + "_regions"] = [round(v, 3) for v in all_]

    # 1. the floor
    env = make()
    fixed = torch.randint(0, 3, (n,), device=dev, dtype=torch.int64).to(torch.uint8)
    graph = env.capture_step(fixed)
    record("step_only", graph.launch)
    graph.close()

    # 2. the path before the device network
    env = make(normalized_obs=True)
    policy = GreedyQPolicy(layers, dev)
    action = torch.zeros(n, dtype=torch.int64, device=dev)
    graph = env.capture_step(action)
    obs_norm = env.obs_norm

    def torch_step():
        action.copy_(policy(obs_norm))
        graph.launch()
    record("torch_policy", torch_step)
    graph.close()

    # 3. / 4. the device network
    env = make()
    record("device_policy_eager", lambda: env.step(policy=qnet))
    env = make()
    graph = env.capture_policy_step(qnet)
    record("device_policy_graph", graph.launch)
    graph.close()

    # 5. the policy kernel alone
    out = torch.zeros(env.ld, dtype=torch.uint8, device=dev)
    record("act_only", lambda: qnet.act(env, out=out))
    tf = FLOP_PER_WORLD * n / (result["act_only"] * 1e-6) / 1e12
    result["act_only_tflops"] = round(tf, 2)
    result["act_only_fraction_of_f32_matrix_peak"] = round(tf / F32_MATRIX_PEAK_TF, 4)
    result["f32_matrix_peak_tflops"] = F32_MATRIX_PEAK_TF
    result["graph_over_torch"] = round(result["device_policy_graph"] / result["torch_policy"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
