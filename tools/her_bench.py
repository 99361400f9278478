#!/usr/bin/env python3
"""Timing of hindsight relabelling of the experience ring (libaqua_her.so) against the composition it replaces.

  relabel  aquaher_relabel at (P, B, H), eagerly and as one captured graph node, beside the same rule written with torch
           indexing on the device (a chain of small kernels: clamps, gathers, selects, Philox rounds in int64, float64
           arithmetic), checked to give the same staged rows before it is timed, and beside aquarpl_draw of the same P B
           samples, the launch that precedes the relabelling in the loops (the launch floor).  The ring is synthetic: 1 024
           worlds, 64 rounds, 2 % of the steps end an episode, 2 % are no experience.
  loop     DQNLoop (1 024 worlds) and PopulationLoop (16 x 1 024) as one graph without and with hindsight=; without is the
           chain as it was, node for node.

HIP events around --calls calls, the median of --windows windows, the variants alternating window by window; every window
is reported.  One JSON line per measurement on stdout.

    python tools/her_bench.py [--calls 200] [--windows 5] [--shapes 1x64x32,16x64x32,1024x64x32,1x65536x32] [--no-loop]
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
RATIO = 0.8
M32 = 0xFFFFFFFF


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
    """a full ring as HindsightReplay reads a DeviceReplayRing, cursor mid-ring"""
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


def torch_philox(key, j, tick, stream):
    """Philox4x32-10 in int64 tensors (products wrap modulo 2^64, which keeps their low 64 bits) -> words 0 and 1.
    key, tick: int64 [n] (uint64 bit patterns); j: int64 [n]"""
    k0, k1 = key & M32, (key >> 32) & M32
    c0, c1, c2 = j & M32, (j >> 32) & M32, tick & M32
    c3 = ((tick >> 32) & 0xFFFF) | (stream << 24)
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & M32) ^ c1 ^ k0, p1 & M32, ((p0 >> 32) & M32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1


def torch_relabel(ring, idx, H, thr, t, seed, out):
    """aquaher_relabel's rule (csrc/aqua_her.h) with torch indexing, for one scalar key.  Fixed shapes, no host read: it can be
    captured.  t: int64 [P] on the device; out: (s, a, r, s2, d, ok, k, m)"""
    cap, N = ring.capacity, ring.env.num_envs
    P, B = idx.shape
    c = idx.reshape(-1).long()
    inside = (c >= 0) & (c < cap)
    c = c.clamp(0, cap - 1)
    cursor = ring.header[0]
    ring_ok = (cursor >= 0) & (cursor < cap) & (cursor % N == 0)
    age = torch.remainder(cursor - N - (c - c % N), cap) // N
    valid = inside & ring_ok & (ring.ok[c] != 0)
    walking, M = valid, torch.zeros_like(c)
    for k in range(H):
        slot = (c + k * N) % cap
        walking = walking & (age >= k) & (ring.ok[slot] != 0) & (ring.d[slot] == 0)
        M = torch.where(walking, torch.full_like(M, k + 1), M)
    j = torch.arange(B, device=c.device).repeat(P)
    tick = (t + 1).repeat_interleave(B)
    r0, r1 = torch_philox(torch.full_like(c, seed), j, tick, 8)
    chosen = (M > 0) & (r0 < thr)
    k = (r1 * M) >> 32
    goal = torch.where(chosen, (c + k * N) % cap, c)
    g = ring.s2[0:2][:, goal]
    s_rows, s2_rows = ring.s[:, c].clone(), ring.s2[:, c].clone()

    def gap(q):
        dx, dy = q[0].double() - g[0].double(), q[1].double() - g[1].double()
        return 100.0 * torch.sqrt(dx * dx + dy * dy) - 5.0
    gap_prev, gap_new = gap(s_rows), gap(s2_rows)
    hit = gap_new <= 0
    r_new = torch.where(hit, torch.full_like(gap_new, 10.0), 0.7 * (gap_prev - gap_new)).float()
    s_rows[3:5] = torch.where(chosen, g, s_rows[3:5])
    s2_rows[3:5] = torch.where(chosen, g, s2_rows[3:5])
    zero = torch.zeros((), dtype=torch.float32, device=c.device)
    s, a, r, s2, d, ok, kk, mm = out
    s.copy_(torch.where(valid, s_rows, zero))
    s2.copy_(torch.where(valid, s2_rows, zero))
    a.copy_(torch.where(valid, ring.a[c], torch.zeros_like(ring.a[c])))
    r.copy_(torch.where(valid, torch.where(chosen, r_new, ring.r[c]), zero))
    code = torch.where(chosen, hit.to(torch.uint8) * 3, ring.d[c])
    d.copy_(torch.where(valid, code, torch.zeros_like(code)))
    ok.copy_(valid.to(torch.uint8))
    kk.copy_(torch.where(chosen, k + 1, torch.zeros_like(k)).to(torch.uint8))
    mm.copy_(M.to(torch.uint8))


def bench_relabel(ring, P, B, H, calls, count):
    from aquaticgymenv_amd import _her_capi, _replay_capi
    from aquaticgymenv_amd.hindsight import HindsightReplay
    rng = np.random.RandomState(P + B + H)
    idx = torch.from_numpy(rng.randint(-1, ring.capacity, (P, B)).astype(np.int32)).to(DEV)
    her = HindsightReplay(ring, B, networks=P, horizon=H, ratio=RATIO)
    other = her._staging()
    t = torch.from_numpy(rng.randint(0, 1000, P).astype(np.int64)).to(DEV)
    seed = 12345
    thr = _her_capi.threshold(RATIO)
    relabel = lambda: her._launch(idx, t, seed, None, her._rows)                   # noqa: E731
    composed = lambda: torch_relabel(ring, idx, H, thr, t, seed, other)            # noqa: E731
    t_dev, drawn = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty(P * B, dtype=torch.int32, device=DEV)

    def draw():
        _replay_capi.check(_replay_capi.lib.aquarpl_draw(ring.header.data_ptr(), ring.ok.data_ptr(), ring.capacity, t_dev.data_ptr(), 3,
                                                         drawn.data_ptr(), P * B, torch.cuda.current_stream().cuda_stream), "aquarpl_draw")
    relabel()
    composed()
    torch.cuda.synchronize()
    for mine, theirs in zip(her._rows, other):                 # the yardstick computes the same thing
        assert torch.equal(mine, theirs)
    share = float((her.k > 0).float().mean())
    for mode in ("eager", "graph"):
        keep = []
        if mode == "graph":
            relabel, k1 = captured(relabel)
            composed, k2 = captured(composed)
            draw, k3 = captured(draw)
            keep = [k1, k2, k3]
        med, raw = windows({"relabel": relabel, "torch": composed, "draw": draw}, calls, count)
        emit(what="relabel", mode=mode, P=P, B=B, H=H, calls=calls, windows=count, relabelled_share=share, relabel_us=med["relabel"],
             torch_us=med["torch"], draw_us=med["draw"], draw_min_max_us=[min(raw["draw"]), max(raw["draw"])],
             relabel_min_max_us=[min(raw["relabel"]), max(raw["relabel"])], torch_min_max_us=[min(raw["torch"]), max(raw["torch"])], raw=raw)
        del keep


def dqn_loop(hindsight, B, H):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.hindsight import HindsightReplay
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.trainer import DQNLoop
    qnet = QNetwork(L.glorot_layers(3), DEV)
    learner = DQNLearner(qnet, lr=1e-4, seed=3)
    env = BatchedAqua(WORLDS, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    tracker = EpisodeTracker(env, epsilon=(0.1, 0.05, 10000))
    ring = DeviceReplayRing(env, 16 * WORLDS)
    her = HindsightReplay(ring, B, horizon=H, ratio=RATIO) if hindsight else None
    return DQNLoop(env, qnet, learner, ring, tracker, B, hindsight=her).capture()


def population_loop(hindsight, P, seg, B, H):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.hindsight import HindsightReplay
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
    ring = DeviceReplayRing(env, 16 * P * seg)
    her = HindsightReplay(ring, B, networks=P, horizon=H, ratio=RATIO) if hindsight else None
    return PopulationLoop(env, bank, learners, ring, tracker, B, segments=st, hindsight=her).capture()


def bench_loops(B, H, calls, count):
    for what, make in (("dqn_loop", lambda h: dqn_loop(h, B, H)), ("population_loop", lambda h: population_loop(h, 16, WORLDS, B, H))):
        graphs = {"plain": make(False), "hindsight": make(True)}
        for g in graphs.values():                              # past the first rounds, in which no walk is longer than a step
            for _ in range(8):
                g.launch()
        med, raw = windows({name: g.launch for name, g in graphs.items()}, calls, count)
        emit(what=what, mode="graph", B=B, H=H, calls=calls, windows=count, plain_us=med["plain"], hindsight_us=med["hindsight"],
             difference_us=med["hindsight"] - med["plain"], plain_min_max_us=[min(raw["plain"]), max(raw["plain"])],
             hindsight_min_max_us=[min(raw["hindsight"]), max(raw["hindsight"])], raw=raw)
        for g in graphs.values():
            g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="1x64x32,16x64x32,1024x64x32,1x65536x32", help="P x B x H of the relabel measurements")
    ap.add_argument("--batch", type=int, default=64, help="samples per network of the loop measurements")
    ap.add_argument("--horizon", type=int, default=32, help="H of the loop measurements")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the relabelling has no CPU path")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    ring = synthetic_ring()
    for shape in args.shapes.split(","):
        P, B, H = (int(v) for v in shape.split("x"))
        bench_relabel(ring, P, B, H, args.calls, args.windows)
    if not args.no_loop:
        bench_loops(args.batch, args.horizon, args.calls, args.windows)


if __name__ == "__main__":
    main()
