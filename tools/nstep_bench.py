#!/usr/bin/env python3
"""Timing of the n-step fold of the experience ring (libaqua_nstep.so) against the composition it replaces.

  fold     aquanst_fold at (P, B, n), eagerly and as one captured graph node, beside the same fold written with torch
           indexing on the device (a chain of small kernels: clamps, gathers, selects, float64 products), checked to give
           the same staged rows before it is timed, and beside aquarpl_draw of the same P B samples, the launch that
           precedes the fold in the loops.  The ring is synthetic: 1 024 worlds, 64 rounds, 2 % of the steps end an
           episode, 2 % are no experience.
  loop     DQNLoop (1 024 worlds) and PopulationLoop (16 x 1 024) as one graph with n_step 1 and with n_step 3; n_step 1
           is the chain without the fold, node for node.

HIP events around --calls calls, the median of --windows windows, the variants alternating window by window; every window
is reported.  One JSON line per measurement on stdout.

    python tools/nstep_bench.py [--calls 200] [--windows 5] [--shapes 1x64x3,16x64x3,1024x64x5,1x65536x3] [--no-loop]
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import _learner as L

DEV = "cuda:0"
WORLDS, ROUNDS = 1024, 64


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


def synthetic_ring(seed=1):
    """a full ring as NStepReturns reads a DeviceReplayRing, cursor mid-ring"""
    rng = np.random.RandomState(seed)
    cap = WORLDS * ROUNDS
    ring = types.SimpleNamespace(torch=torch, device=torch.device(DEV), capacity=cap, _kind=0,
                                 env=types.SimpleNamespace(num_envs=WORLDS, continuous=False),
                                 header=torch.tensor([17 * WORLDS, cap, 16 * WORLDS, 81], dtype=torch.int64, device=DEV))
    host = dict(s=rng.rand(5, cap).astype(np.float32), s2=rng.rand(5, cap).astype(np.float32), r=(rng.rand(cap) * 2 - 1).astype(np.float32),
                a=rng.randint(0, 3, cap).astype(np.uint8), d=(rng.randint(1, 4, cap) * (rng.rand(cap) < 0.02)).astype(np.uint8),
                ok=(rng.rand(cap) < 0.98).astype(np.uint8))
    for k, v in host.items():
        setattr(ring, k, torch.from_numpy(v).to(DEV))
    return ring


def torch_fold(ring, idx, n, g, out):
    """aquanst_fold's window rule and return (csrc/aqua_nstep.h) with torch indexing, for one scalar gamma; g: float64
    float32(gamma).  Fixed shapes, no host read: it can be captured.  out: (s, a, r, s2, d, ok, length)"""
    cap, N = ring.capacity, ring.env.num_envs
    c = idx.reshape(-1).long()
    inside = (c >= 0) & (c < cap)
    c = c.clamp(0, cap - 1)
    cursor = ring.header[0]
    ring_ok = (cursor >= 0) & (cursor < cap) & (cursor % N == 0)
    age = torch.remainder(cursor - N - (c - c % N), cap) // N
    walking = inside & ring_ok
    valid = torch.zeros_like(walking)
    last, length, code = c.clone(), torch.zeros_like(c), torch.zeros_like(c)
    acc = torch.zeros(c.shape, dtype=torch.float64, device=c.device)
    pw = 1.0
    for k in range(n):
        slot = (c + k * N) % cap
        go = walking & (age >= k) & (ring.ok[slot] != 0)
        r = ring.r[slot].double()
        if k > 0:
            pw = pw * g                                        # (a Python float: every product rounded in double)
        acc = torch.where(go, r if k == 0 else acc + pw * r, acc)
        d = ring.d[slot].long()
        end = go & ((d != 0) | (k == n - 1))
        valid = valid | end
        last = torch.where(end, slot, last)
        length = torch.where(end, torch.full_like(length, k + 1), length)
        code = torch.where(end, d, code)
        walking = go & ~end
    zero = torch.zeros((), dtype=torch.float32, device=c.device)
    s, a, r, s2, d, ok, ln = out
    s.copy_(torch.where(valid, ring.s[:, c], zero))
    s2.copy_(torch.where(valid, ring.s2[:, last], zero))
    a.copy_(torch.where(valid, ring.a[c], torch.zeros_like(ring.a[c])))
    r.copy_(torch.where(valid, acc, torch.zeros_like(acc)).float())
    d.copy_(torch.where(valid, code, torch.zeros_like(code)).to(torch.uint8))
    ok.copy_(valid.to(torch.uint8))
    ln.copy_(length.to(torch.uint8))


def bench_fold(ring, P, B, n, calls, count):
    from aquaticgymenv_amd.nstep import NStepReturns
    rng = np.random.RandomState(P + B + n)
    idx = torch.from_numpy(rng.randint(-1, ring.capacity, (P, B)).astype(np.int32)).to(DEV)
    nstep = NStepReturns(ring, n, B, networks=P)
    other = nstep._staging()
    gamma = 0.98
    g = float(np.float32(gamma))
    fold = lambda: nstep.fold(idx, gamma=gamma)                # noqa: E731
    composed = lambda: torch_fold(ring, idx, n, g, other)      # noqa: E731
    from aquaticgymenv_amd import _replay_capi
    t_dev, drawn = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty(P * B, dtype=torch.int32, device=DEV)

    def draw():
        _replay_capi.check(_replay_capi.lib.aquarpl_draw(ring.header.data_ptr(), ring.ok.data_ptr(), ring.capacity, t_dev.data_ptr(), 3,
                                                         drawn.data_ptr(), P * B, torch.cuda.current_stream().cuda_stream), "aquarpl_draw")
    fold()
    composed()
    torch.cuda.synchronize()
    for mine, theirs in zip(nstep._rows, other):               # the yardstick computes the same thing
        assert torch.equal(mine, theirs)
    share = float(nstep.ok.float().mean())
    for mode in ("eager", "graph"):
        keep = []
        if mode == "graph":
            fold, k1 = captured(fold)
            composed, k2 = captured(composed)
            draw, k3 = captured(draw)
            keep = [k1, k2, k3]
        med, raw = windows({"fold": fold, "torch": composed, "draw": draw}, calls, count)
        emit(what="fold", mode=mode, P=P, B=B, n=n, calls=calls, windows=count, valid_share=share, fold_us=med["fold"], torch_us=med["torch"],
             draw_us=med["draw"], draw_min_max_us=[min(raw["draw"]), max(raw["draw"])], fold_min_max_us=[min(raw["fold"]), max(raw["fold"])], torch_min_max_us=[min(raw["torch"]), max(raw["torch"])], raw=raw)
        del keep


def dqn_loop(n_step, B):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.trainer import DQNLoop
    qnet = QNetwork(L.glorot_layers(3), DEV)
    learner = DQNLearner(qnet, lr=1e-4, seed=3)
    env = BatchedAqua(WORLDS, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    tracker = EpisodeTracker(env, epsilon=(0.1, 0.05, 10000))
    return DQNLoop(env, qnet, learner, DeviceReplayRing(env, 16 * WORLDS), tracker, B, n_step=n_step).capture()


def population_loop(n_step, P, seg, B):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    from aquaticgymenv_amd.trainer import PopulationLoop
    env = BatchedAqua(P * seg, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    bank = QNetworkBank([L.glorot_layers(100 + p) for p in range(P)], seg, DEV)
    tracker = EpisodeTracker(env)
    st = SegmentTracker(tracker, seg, P, window=100, epsilon=(0.1, 0.05, 10000))
    bank.epsilon = st.epsilon
    learners = DQNLearnerBank(bank, lr=1e-4, seed=3)
    return PopulationLoop(env, bank, learners, DeviceReplayRing(env, 16 * P * seg), tracker, B, segments=st, n_step=n_step).capture()


def bench_loops(B, calls, count):
    for what, make in (("dqn_loop", lambda n: dqn_loop(n, B)), ("population_loop", lambda n: population_loop(n, 16, WORLDS, B))):
        graphs = {"n_step_1": make(1), "n_step_3": make(3)}
        for g in graphs.values():                              # past the first rounds, in which no window of three closes
            for _ in range(8):
                g.launch()
        med, raw = windows({name: g.launch for name, g in graphs.items()}, calls, count)
        emit(what=what, mode="graph", B=B, calls=calls, windows=count, n_step_1_us=med["n_step_1"], n_step_3_us=med["n_step_3"],
             difference_us=med["n_step_3"] - med["n_step_1"], n_step_1_min_max_us=[min(raw["n_step_1"]), max(raw["n_step_1"])],
             n_step_3_min_max_us=[min(raw["n_step_3"]), max(raw["n_step_3"])], raw=raw)
        for g in graphs.values():
            g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="1x64x3,16x64x3,1024x64x5,1x65536x3", help="P x B x n of the fold measurements")
    ap.add_argument("--batch", type=int, default=64, help="samples per network of the loop measurements")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the fold has no CPU path")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    ring = synthetic_ring()
    for shape in args.shapes.split(","):
        P, B, n = (int(v) for v in shape.split("x"))
        bench_fold(ring, P, B, n, args.calls, args.windows)
    if not args.no_loop:
        bench_loops(args.batch, args.calls, args.windows)


if __name__ == "__main__":
    main()
