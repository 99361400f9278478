#!/usr/bin/env python3
"""Timing of the learner bank (libaqua_lbank.so) against what it replaces.

  update   one aqualbank_update_f32 of P networks  vs  the P sequential aqualrn_update_f32 calls of the same minibatches
  draw     one aqualbank_draw of P networks         vs  P aquarpl_draw calls on the same ring
  loop     one PopulationLoop graph (P networks x W worlds, one batch)  vs  P DQNLoop graphs (W worlds each) one after the other

The yardstick is the path that exists without the library, not the code under test.  HIP events around --calls calls, the
median of --windows windows, the two variants alternating window by window; update and draw are timed eagerly and as one
captured graph each.  Before anything is timed, both variants run once from the same state and must leave the same bits.
One JSON line per measurement on stdout.

    python tools/lbank_bench.py [--calls 200] [--windows 5] [--shapes 1x64,16x64,256x64,1024x64,16x4096] [--no-loop]
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

from tests import _lbank as K
from tests import _learner as L

DEV = "cuda:0"
N_WORLDS, ROUNDS = 1024, 64          # the ring of the update / draw measurements: 64 rounds of 1 024 worlds


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


def bench_update(run, P, B, calls, count):
    cap = N_WORLDS * ROUNDS
    ring_np = L.float_ring(cap, cap, 5, bad_ok=0.02)
    ring = L.DeviceRing(torch, ring_np, DEV)
    st = K.make_state(P, 7)
    hyper = K.hypers(P)
    hyper[:, 2] *= 0.01                                        # small steps: thousands of updates on one ring stay finite
    hd = run.hyper_dev(hyper)
    idx = torch.as_tensor(np.random.RandomState(1).randint(0, cap, (P, B)).astype(np.int32)).to(DEV)
    a, b = K.to_device(torch, st, B, DEV), K.to_device(torch, st, B, DEV)
    bank = lambda: run.bank_update(a, ring, idx, B, 0, hd)
    singles = lambda: run.single_updates(b, ring, idx, B, 0, hyper)
    bank()
    singles()
    diff = K.differing(K.read(torch, a), K.read(torch, b))
    if diff:
        raise SystemExit("update P=%d B=%d: the bank and the single calls differ in %s" % (P, B, diff))
    med, raw = windows({"bank": bank, "singles": singles}, calls, count)
    emit(what="update", mode="eager", P=P, B=B, calls=calls, windows=count, bank_us=med["bank"], singles_us=med["singles"],
         ratio=med["singles"] / med["bank"], raw=raw)
    gb, keep_b = captured(bank)
    gs, keep_s = captured(singles)
    med, raw = windows({"bank": gb, "singles": gs}, calls, count)
    diff = K.differing(K.read(torch, a), K.read(torch, b))     # the same number of updates on both sides, replays included
    emit(what="update", mode="graph", P=P, B=B, calls=calls, windows=count, bank_us=med["bank"], singles_us=med["singles"],
         ratio=med["singles"] / med["bank"], same_bits_after=not diff, raw=raw)
    del keep_b, keep_s


def bench_draw(run, P, B, calls, count):
    from aquaticgymenv_amd import _replay_capi
    cap, seg = N_WORLDS * ROUNDS, max(N_WORLDS // P, 1)
    header = torch.as_tensor(np.array([0, cap, 0, 0], dtype=np.int64)).to(DEV)
    ok = torch.as_tensor((np.random.RandomState(2).rand(cap) >= 0.02).astype(np.uint8)).to(DEV)
    t = torch.zeros(P, dtype=torch.int64, device=DEV)
    seeds = torch.arange(P, dtype=torch.int64, device=DEV)
    out_b = torch.full((P, B), -1, dtype=torch.int32, device=DEV)
    out_s = torch.full((P, B), -1, dtype=torch.int32, device=DEV)

    def bank():
        run.bank.check(run.bank.lib.aqualbank_draw(header.data_ptr(), ok.data_ptr(), cap, N_WORLDS, seg, P, t.data_ptr(), seeds.data_ptr(),
                                                   out_b.data_ptr(), B, run._stream()), "aqualbank_draw")

    def singles():
        s = run._stream()
        for p in range(P):
            _replay_capi.check(_replay_capi.lib.aquarpl_draw(header.data_ptr(), ok.data_ptr(), cap, t[p:].data_ptr(), p, out_s[p].data_ptr(),
                                                             B, s), "aquarpl_draw")
    bank()
    torch.cuda.synchronize()
    want = K.draw_model(list(range(P)), [0] * P, B, cap, ok.cpu().numpy(), cap, N_WORLDS, seg)
    if not np.array_equal(out_b.cpu().numpy(), want):
        raise SystemExit("draw P=%d B=%d differs from the model" % (P, B))
    for mode, pair in (("eager", (bank, singles)), ("graph", None)):
        if pair is None:
            gb, kb = captured(bank)
            gs, ks = captured(singles)
            pair = (gb, gs)
        med, raw = windows({"bank": pair[0], "singles": pair[1]}, calls, count)
        emit(what="draw", mode=mode, P=P, B=B, calls=calls, windows=count, bank_us=med["bank"], singles_us=med["singles"],
             ratio=med["singles"] / med["bank"], raw=raw)


def bench_loop(P, W, B, calls, count):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.trainer import DQNLoop, PopulationLoop
    nets = [L.glorot_layers(100 + p) for p in range(P)]
    env = BatchedAqua(P * W, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    bank = QNetworkBank(nets, W, DEV)
    bank.epsilon = torch.full((P,), 0.1, dtype=torch.float32, device=DEV)
    learners = DQNLearnerBank(bank, lr=1e-4, seed=3)
    pop = PopulationLoop(env, bank, learners, DeviceReplayRing(env, 64 * P * W), EpisodeTracker(env), B).capture()
    chains = []
    for p in range(P):
        e = BatchedAqua(W, obstacles=True, seed=3 + p, auto_reset="next_step", normalized_obs=True, device=DEV)
        e.reset()
        q = QNetwork(nets[p], DEV)
        chains.append(DQNLoop(e, q, DQNLearner(q, lr=1e-4, seed=3 + p), DeviceReplayRing(e, 64 * W), EpisodeTracker(e, epsilon=(0.1, 0.1, 1.0)),
                              B).capture())

    def singles():
        for g in chains:
            g.launch()
    med, raw = windows({"population": pop.launch, "chains": singles}, calls, count)
    emit(what="loop", mode="graph", P=P, worlds_per_network=W, B=B, calls=calls, windows=count, population_us=med["population"],
         chains_us=med["chains"], ratio=med["chains"] / med["population"], raw=raw)
    pop.close()
    for g in chains:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="1x64,16x64,256x64,1024x64,16x4096")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the learner bank has no CPU path")
    run = K.Runner(torch, DEV)
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    for shape in args.shapes.split(","):
        P, B = (int(v) for v in shape.split("x"))
        bench_update(run, P, B, args.calls, args.windows)
        bench_draw(run, P, B, args.calls, args.windows)
    if not args.no_loop:
        bench_loop(16, 1024, 64, args.calls, args.windows)


if __name__ == "__main__":
    main()
