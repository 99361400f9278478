#!/usr/bin/env python3
"""Timing of the per-segment episode bookkeeping (libaqua_segments.so) against the host refresh it replaces.

  launch   one aquaseg_account behind one aquaep_after_step_f32, eagerly and as one captured graph, against the accounting
           call alone: the difference is the new launch.  The rows end a fixed share of the worlds every step.
  loop     PopulationLoop as one graph with segments= (eleven kernels) and without (ten)
  refresh  the host refresh of examples/dqn_population.py --host-refresh, as it was the only way before: read the counter
           and the new records back, np.bincount(world // seg) on the host, P floats of epsilon back to the device.  One
           refresh after one step; the example ran it every --refresh iterations.

The yardstick is the path that exists without the library.  HIP events around --calls calls, the median of --windows
windows, the variants alternating window by window.  One JSON line per measurement on stdout.

    python tools/segments_bench.py [--calls 200] [--windows 5] [--shapes 16x1024,4096x16] [--no-loop]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import _learner as L
from tests import _segments as S

DEV = "cuda:0"


def windows(variants, calls, count):
    """variants: {name: callable queueing ONE call} -> {name: median microseconds per call}, alternating per window"""
    times = {name: [] for name in variants}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in variants.values():                               # untimed first calls
        fn()
    torch.cuda.synchronize()
    for _ in range(count):
        for name, fn in variants.items():
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(1000.0 * start.elapsed_time(stop) / calls)
    return {name: statistics.median(v) for name, v in times.items()}, times


def captured(fn):
    """fn (queueing launches on the current stream) as one torch.cuda.CUDAGraph -> its replay"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay, g


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_launch(P, seg, share, calls, count):
    """every step ends `share` of the worlds"""
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.segments import SegmentTracker
    n = P * seg
    rng = np.random.RandomState(1)
    term = np.where(rng.random_sample(n) < share, rng.randint(1, 4, n), 0).astype(np.uint8)
    pairs = []
    for _ in range(2):
        rows = S.Rows(torch, n, 0, DEV)
        rows.set(rng.uniform(-1.0, 1.0, n), term)
        pairs.append((rows, EpisodeTracker(rows)))
    st = SegmentTracker(pairs[0][1], seg, P, window=100, epsilon=(1.0, 0.05, 10000))
    both, alone = st.after_step, pairs[1][1].after_step
    for mode in ("eager", "graph"):
        if mode == "graph":
            both, keep_a = captured(both)
            alone, keep_b = captured(alone)
        med, raw = windows({"with_segments": both, "accounting_alone": alone}, calls, count)
        emit(what="launch", mode=mode, P=P, seg=seg, ending_per_step=int((term != 0).sum()), calls=calls, windows=count,
             with_segments_us=med["with_segments"], accounting_alone_us=med["accounting_alone"],
             launch_us=med["with_segments"] - med["accounting_alone"], raw=raw)
    got = st.counts()
    assert got["missed"] == 0 and got["stray"] == 0 and sum(r["episodes"] for r in got["segments"]) == pairs[0][1].counts()["episodes"]

    # the host refresh after one step, wall clock: it synchronises, so events around it would measure the same
    rows, tracker = pairs[1]
    eps = torch.ones(P, dtype=torch.float32, device=DEV)
    episodes, seen, decay = np.zeros(P, dtype=np.int64), tracker.counts()["episodes"], (0.05 / 1.0) ** (1.0 / 10000)
    times = []
    for _ in range(count):
        t0 = time.perf_counter()
        for _ in range(calls // 10 or 1):
            tracker.after_step()
            total = tracker.counts()["episodes"]
            new = tracker.last(total - seen)
            episodes += np.bincount(new["world"] // seg, minlength=P)[:P]
            seen = total
            eps.copy_(torch.from_numpy(np.maximum(0.05, 1.0 * decay ** episodes).astype(np.float32)))
        torch.cuda.synchronize()
        times.append(1e6 * (time.perf_counter() - t0) / (calls // 10 or 1))
    emit(what="refresh", mode="host", P=P, seg=seg, ending_per_step=int((term != 0).sum()), windows=count,
         step_and_refresh_us=statistics.median(times), raw=times)


def bench_loop(P, seg, B, calls, count):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    from aquaticgymenv_amd.trainer import PopulationLoop
    base = [L.glorot_layers(100 + p) for p in range(min(P, 16))]
    nets = [base[p % len(base)] for p in range(P)]
    graphs = {}
    for name in ("with_segments", "without"):
        env = BatchedAqua(P * seg, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
        env.reset()
        bank = QNetworkBank(nets, seg, DEV)
        tracker = EpisodeTracker(env)
        st = None
        if name == "with_segments":
            st = SegmentTracker(tracker, seg, P, window=100, epsilon=(0.1, 0.05, 10000))
            bank.epsilon = st.epsilon
        else:
            bank.epsilon = torch.full((P,), 0.1, dtype=torch.float32, device=DEV)
        learners = DQNLearnerBank(bank, lr=1e-4, seed=3)
        graphs[name] = PopulationLoop(env, bank, learners, DeviceReplayRing(env, 16 * P * seg), tracker, B, segments=st).capture()
    med, raw = windows({name: g.launch for name, g in graphs.items()}, calls, count)
    emit(what="loop", mode="graph", P=P, seg=seg, B=B, calls=calls, windows=count, with_segments_us=med["with_segments"],
         without_us=med["without"], difference_us=med["with_segments"] - med["without"], raw=raw)
    for g in graphs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="16x1024,4096x16")
    ap.add_argument("--share", type=float, default=0.01, help="share of the worlds that end in every step of the launch measurement")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the segment tracker has no CPU path")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    for shape in args.shapes.split(","):
        P, seg = (int(v) for v in shape.split("x"))
        bench_launch(P, seg, args.share, args.calls, args.windows)
        if not args.no_loop:
            bench_loop(P, seg, args.batch, args.calls, args.windows)


if __name__ == "__main__":
    main()
