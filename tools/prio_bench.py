#!/usr/bin/env python3
"""Timing of prioritised replay (libaqua_prio.so, aquaticgymenv_amd/priority.py) against the stages it replaces.

  draw     PrioritizedReplay.draw (descent + weights, two launches) beside DQNLearnerBank.draw (the uniform draw, one launch)
           and beside the same rule written with torch: cumsum over the leaves, searchsorted, gather, pow, a row maximum.
  update   PrioritizedReplay.update beside DQNLearnerBank.update at the same (P, B): one multiply and one store per sample more.
  insert   PrioritizedReplay.insert and .set beside the ring's close launch (aquarpl_close) of the same batch, and beside
  set      a torch scatter of the quantised priorities into the leaves.
  loop     PopulationLoop as one graph with and without priorities= (with segments, without a selector).

Every stage eagerly and as one captured graph; HIP events around --calls calls, the median of --windows windows, the variants
alternating window by window; every window is reported.  The ring holds --rounds batched steps and is filled synthetically
(every slot an experience, priorities from exponential TD errors).  One JSON line per measurement on stdout.

    python tools/prio_bench.py [--calls 200] [--windows 5] [--shapes 1x1024x64,16x1024x64,256x64x64] [--rounds 256] [--no-loop]
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


def parts(P, seg, rounds, per=True):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.priority import PrioritizedReplay
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    env = BatchedAqua(P * seg, obstacles=True, seed=3, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    bank = QNetworkBank([L.glorot_layers(100 + p) for p in range(P)], seg, DEV)
    tracker = EpisodeTracker(env)
    st = SegmentTracker(tracker, seg, P, window=100, epsilon=(0.1, 0.05, 10000))
    bank.epsilon = st.epsilon
    learners = DQNLearnerBank(bank, lr=1e-4, seed=3)
    ring = DeviceReplayRing(env, rounds * P * seg)
    return dict(env=env, bank=bank, tracker=tracker, st=st, learners=learners, ring=ring,
                per=PrioritizedReplay(ring, learners, anneal=100000) if per else None)


def fill(p, B, seed=1):
    """a full ring of synthetic experiences, every batch inserted, then priorities from exponential TD errors"""
    ring, per = p["ring"], p["per"]
    rng = np.random.RandomState(seed)
    cap, N = ring.capacity, ring.env.num_envs
    ring.s.copy_(torch.from_numpy(rng.rand(5, cap).astype(np.float32)))
    ring.s2.copy_(torch.from_numpy(rng.rand(5, cap).astype(np.float32)))
    ring.r.copy_(torch.from_numpy((rng.rand(cap) * 2 - 1).astype(np.float32)))
    ring.a.copy_(torch.from_numpy(rng.randint(0, 3, cap).astype(np.uint8)))
    ring.d.copy_(torch.from_numpy((rng.randint(1, 4, cap) * (rng.rand(cap) < 0.02)).astype(np.uint8)))
    ring.ok.fill_(1)
    header = ring.header.clone()
    for r in range(cap // N):
        header[2] = r * N
        per._insert(per.tree, per.pmax, header)
    ring.header.copy_(torch.tensor([0, cap, cap - N, cap // N], dtype=torch.int64))
    per._grow(B)
    for _ in range(8):
        per.draw(B)
        per.td.copy_(torch.from_numpy(rng.exponential(1.0, tuple(per.td.shape)).astype(np.float32)))
        per.set()
        p["learners"].t += 1
    torch.cuda.synchronize()


def torch_rule(per, B):
    """the draw and the set with torch on the leaves alone (no tree: the cumulative sums are rebuilt by every draw)"""
    capi = per._capi
    lay, P = per.layout, per.networks
    leaves = per.tree[:P * lay["stride"][0] * 4].view(torch.int32).reshape(P, lay["stride"][0])[:, :lay["n"][0]].long().clone()
    u01 = torch.rand((P, B), dtype=torch.float64, device=DEV)
    size = float(max(1, lay["n"][0]))
    td = torch.rand((P, B), dtype=torch.float32, device=DEV)
    state = {}

    def draw():
        cum = leaves.cumsum(1)
        T = cum[:, -1:]
        u = (u01 * T.double()).long()
        c = torch.searchsorted(cum, u, right=True).clamp_(max=leaves.shape[1] - 1)
        q = leaves.gather(1, c)
        w = (size * q.double() / T.double().clamp_(min=1.0)).clamp_(min=1e-300).pow(-0.4)
        state["c"], state["w"] = c, (w / w.max(dim=1, keepdim=True).values).float()

    def set_():
        q = ((td.double() + per.eps).pow(per.alpha) * capi.ONE).round().clamp_(1, capi.QMAX).long()
        leaves.scatter_(1, state["c"], q)

    draw()
    return draw, set_


def bench_stages(P, seg, B, rounds, calls, count):
    p = parts(P, seg, rounds)
    fill(p, B)
    per, learners, ring = p["per"], p["learners"], p["ring"]
    view, uniform = ring.learner_view(), torch.full((P, B), -1, dtype=torch.int32, device=DEV)
    t0 = learners.t.clone()
    rule_draw, rule_set = torch_rule(per, B)
    env, s = ring.env, None
    stages = {
        "draw": {"per": lambda: per.draw(B), "uniform": lambda: learners.draw(ring, B, out=uniform), "torch": rule_draw},
        "update": {"per": lambda: per.update(view, B, per.idx), "bank": lambda: learners.update(view, B, per.idx)},
        "insert_set": {"insert": per.insert, "set": per.set, "torch_set": rule_set,
                       "close": lambda: ring._capi.check(ring._close_launch(env.reward.data_ptr(), env.term.data_ptr(), ring._stream()), "aquarpl_close")},
    }
    per.draw(B)
    per.update(view, B, per.idx)
    for what, variants in stages.items():
        for mode in ("eager", "graph"):
            keep, run = [], dict(variants)
            if mode == "graph":
                for name, fn in variants.items():
                    run[name], g = captured(fn)
                    keep.append(g)
            med, raw = windows(run, calls, count)
            emit(what=what, mode=mode, P=P, seg=seg, B=B, rounds=rounds, leaves=per.layout["n"][0], levels=per.layout["levels"], calls=calls,
                 windows=count, us={k: round(v, 3) for k, v in med.items()}, min_max_us={k: [round(min(v), 3), round(max(v), 3)] for k, v in raw.items()})
            del keep
    learners.t.copy_(t0)


def bench_loop(P, seg, B, rounds, calls, count):
    from aquaticgymenv_amd.trainer import PopulationLoop
    graphs = {}
    for name, with_per in (("uniform", False), ("prioritised", True)):
        p = parts(P, seg, rounds, per=with_per)
        graphs[name] = PopulationLoop(p["env"], p["bank"], p["learners"], p["ring"], p["tracker"], B, segments=p["st"], priorities=p["per"]).capture()
    for g in graphs.values():
        for _ in range(8):
            g.launch()
    med, raw = windows({name: g.launch for name, g in graphs.items()}, calls, count)
    emit(what="population_loop", mode="graph", P=P, seg=seg, B=B, rounds=rounds, calls=calls, windows=count, us={k: round(v, 3) for k, v in med.items()},
         difference_us=round(med["prioritised"] - med["uniform"], 3), min_max_us={k: [round(min(v), 3), round(max(v), 3)] for k, v in raw.items()})
    for g in graphs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="1x1024x64,16x1024x64,256x64x64", help="P x seg x B")
    ap.add_argument("--rounds", type=int, default=256, help="batched steps the ring holds")
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: prioritised replay has no CPU path")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    for shape in args.shapes.split(","):
        P, seg, B = (int(v) for v in shape.split("x"))
        bench_stages(P, seg, B, args.rounds, args.calls, args.windows)
        if not args.no_loop:
            bench_loop(P, seg, B, args.rounds, args.calls, args.windows)


if __name__ == "__main__":
    main()
