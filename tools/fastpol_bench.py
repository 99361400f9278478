#!/usr/bin/env python3
"""Timing of the fast acting path (libaqua_fastpol.so: the Q-network's hidden layers on the f16 MFMA, operands split hi / lo)
against the float32 acting kernels, in the same process and on the same buffers.

  act      FastActor.act against QNetwork.act (aquapol_act_f32, P = 1) or QNetworkBank.act (aquabank_act_f32), eagerly and
           as a graph node, at the shapes of tools/policy_bench.py and the bank's: (P, seg) = (1, 262144), (2, 131072),
           (150, 1024), (4096, 16)
  step     policy + step on BatchedAqua (BENCH8, next_step), env.step(policy=...) eagerly and capture_policy_step() as one
           graph, with the fast actor and with the float32 network, at 262 144 worlds
  refresh  FastActor.refresh() alone at P = 1, 256, 4096
  loop     PopulationLoop as one graph with actor= and without, segments= and selector= in both, at (16, 1024)

HIP events around --calls calls; the figure is the MEDIAN of --windows windows, the variants alternating window by window,
and `spread` is max - min of the windows.  One JSON line per measurement on stdout.  To time a tuning build of the library
(-DAQUA_FAST_TUNING -DAQUA_FAST_WAVES_PER_SIMD=1 ...), name it in AQUA_FASTPOL_LIB.

    python tools/fastpol_bench.py [--calls 200] [--windows 5] [--only act,step,refresh,loop]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import _learner as L

DEV = "cuda:0"
ACT_SHAPES = ((1, 262144), (2, 131072), (150, 1024), (4096, 16))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def windows(variants, calls, count):
    """variants: {name: callable queueing ONE call} -> {name: (median us per call, max - min of the windows, the windows)}"""
    times = {name: [] for name in variants}
    for fn in variants.values():                               # untimed first calls
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(count):
        for name, fn in variants.items():
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(1000.0 * start.elapsed_time(stop) / calls)
    return {name: (statistics.median(v), max(v) - min(v), [round(x, 3) for x in v]) for name, v in times.items()}


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay, g


def golden(tag="with_obs"):
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    return [(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)]


def networks(P):
    base = [L.glorot_layers(100 + p) for p in range(min(P, 16))]
    return [base[p % len(base)] for p in range(P)]


def report(what, mode, res, **kw):
    (fast, fast_spread, fast_w), (f32, f32_spread, f32_w) = res["fast"], res["f32"]
    emit(what=what, mode=mode, fast_us=round(fast, 3), f32_us=round(f32, 3), fast_spread_us=round(fast_spread, 3), f32_spread_us=round(f32_spread, 3),
         speedup=round(f32 / fast, 3), beats_by_more_than_the_spreads=bool(f32 - fast > fast_spread + f32_spread), fast_windows=fast_w,
         f32_windows=f32_w, **kw)


def bench_act(P, seg, calls, count):
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    n = P * seg
    f32 = QNetwork(golden(), DEV) if P == 1 else QNetworkBank(networks(P), seg, DEV)
    fast = FastActor(f32)
    buf = torch.rand((5, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out = {name: torch.zeros(n, dtype=torch.uint8, device=DEV) for name in ("fast", "f32")}
    variants = {"fast": lambda: fast.act(buf, out=out["fast"]), "f32": lambda: f32.act(buf, out=out["f32"])}
    report("act", "eager", windows(variants, calls, count), P=P, seg=seg, worlds=n, calls=calls, windows=count)
    keep = []
    for name in list(variants):
        variants[name], g = captured(variants[name])
        keep.append(g)
    report("act", "graph", windows(variants, calls, count), P=P, seg=seg, worlds=n, calls=calls, windows=count)
    emit(what="act_agreement", P=P, seg=seg, actions_equal_share=float((out["fast"] == out["f32"]).float().mean()))


def bench_step(n, calls, count):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.qpolicy import QNetwork
    qnet = QNetwork(golden(), DEV)
    policies = {"fast": FastActor(qnet), "f32": qnet}

    def make():
        env = BatchedAqua(n, obstacles=presets.BENCH8, seed=0, auto_reset="next_step", device=DEV)
        env.reset()
        return env
    envs = {name: make() for name in policies}
    eager = {name: (lambda name=name: envs[name].step(policy=policies[name])) for name in policies}
    report("policy_plus_step", "eager", windows(eager, calls, count), worlds=n, calls=calls, windows=count)
    envs = {name: make() for name in policies}
    graphs = {name: envs[name].capture_policy_step(policies[name]) for name in policies}
    report("policy_plus_step", "graph", windows({name: g.launch for name, g in graphs.items()}, calls, count), worlds=n, calls=calls, windows=count)
    for g in graphs.values():
        g.close()


def bench_refresh(P, calls, count):
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.qbank import QNetworkBank
    fast = FastActor(QNetworkBank(networks(P), 16, DEV))
    for mode in ("eager", "graph"):
        fn, keep = fast.refresh, None
        if mode == "graph":
            fn, keep = captured(fast.refresh)
        med, spread, raw = windows({"refresh": fn}, calls, count)["refresh"]
        moved = P * (19216 + 21776)                            # the float32 blob read, the fast blob written; the one 43 KB map stays in cache
        emit(what="refresh", mode=mode, P=P, refresh_us=round(med, 3), spread_us=round(spread, 3), bytes_moved=moved,
             bytes_per_s=moved / (med * 1e-6), windows_us=raw)


def bench_loop(P, seg, B, calls, count):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.pbt import PopulationSelector
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    from aquaticgymenv_amd.trainer import PopulationLoop
    graphs = {}
    for name in ("fast", "f32"):
        env = BatchedAqua(P * seg, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
        env.reset()
        bank = QNetworkBank(networks(P), seg, DEV)
        tracker = EpisodeTracker(env)
        st = SegmentTracker(tracker, seg, P, window=100, epsilon=(0.1, 0.05, 10000))
        bank.epsilon = st.epsilon
        learners = DQNLearnerBank(bank, lr=1e-4, seed=3)
        sel = PopulationSelector(learners, st, fraction=0.25, ready=100)
        graphs[name] = PopulationLoop(env, bank, learners, DeviceReplayRing(env, 16 * P * seg), tracker, B, segments=st, selector=sel,
                                      actor=FastActor(bank) if name == "fast" else None).capture()
    report("population_loop", "graph", windows({name: g.launch for name, g in graphs.items()}, calls, count), P=P, seg=seg, B=B, calls=calls,
           windows=count, kernels_fast=14, kernels_f32=13)
    for g in graphs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--only", default="act,step,refresh,loop")
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the fast acting path has no CPU path")
    from aquaticgymenv_amd import _fastpol_capi
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, library=_fastpol_capi.LIB_PATH)
    only = set(filter(None, args.only.split(",")))
    if "act" in only:
        for P, seg in ACT_SHAPES:
            bench_act(P, seg, args.calls, args.windows)
    if "step" in only:
        bench_step(262144, args.calls, args.windows)
    if "refresh" in only:
        for P in (1, 256, 4096):
            bench_refresh(P, args.calls, args.windows)
    if "loop" in only:
        bench_loop(16, 1024, args.batch, args.calls, args.windows)


if __name__ == "__main__":
    main()
