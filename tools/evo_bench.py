#!/usr/bin/env python3
"""Timing of evolution strategies on a Q-network bank (libaqua_evo.so, aquaticgymenv_amd/evolution.py) against the same
rule written with torch.

  ask, fitness, tell   EvolutionStrategy.ask() (one launch), .fitness(tracker) (three) and .tell() (two), eagerly and as a
                       captured graph, on a synthetic log in which every world has finished one episode
  torch                a straightforward composition on the device, no host read: a torch.randn perturbation kept for the
                       tell and scattered through perm into the bank's blob; index_add_ sums and counts of the log per
                       segment; argsort-of-argsort ranks (ties by index), a matrix product with the kept noise and Adam in
                       float32.  It is not the same arithmetic: it stores H x 4739 floats of noise and is not reproducible
                       bit for bit
  generation           one whole generation(env) -- ask, one episode per world under env.step(policy=bank), fitness, tell --
                       wall clock, with the environment's steps and the polls of the episode counter in it

HIP events around --calls calls, the median of --windows windows, the variants alternating window by window.  One JSON line
per measurement on stdout.

    python tools/evo_bench.py [--calls 200] [--windows 5] [--shapes 17x1024,257x64,4095x16] [--no-generation]
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

from tests import _qbank as B
from tests import _segments as S

DEV = "cuda:0"
PARAMS = 4739


def emit(**kw):
    print(json.dumps(kw), flush=True)


def windows(variants, calls, count):
    """variants: {name: callable queueing ONE call} -> ({name: median microseconds per call}, raw), alternating per window"""
    times = {name: [] for name in variants}
    for fn in variants.values():                               # untimed first calls
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
    return {name: statistics.median(v) for name, v in times.items()}, times


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay, g


def population(P, seg, seed=3):
    """an EvolutionStrategy over a bank of P networks and a once-tracker whose log says every world has ended"""
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.evolution import EvolutionStrategy
    from aquaticgymenv_amd.qbank import QNetworkBank
    base = [B.random_layers(100 + p) for p in range(min(P, 8))]
    bank = QNetworkBank([base[p % len(base)] for p in range(P)], seg, DEV)
    es = EvolutionStrategy(bank, sigma=0.05, lr=0.01, seed=seed)
    n = P * seg
    tracker = EpisodeTracker(S.Rows(torch, n, 0, DEV), capacity=n, once=True)
    rng = np.random.RandomState(seed)
    tracker.log_ret.copy_(torch.from_numpy((rng.randn(n) * 30).astype(np.float32)))
    tracker.log_code.copy_(torch.from_numpy(rng.randint(1, 4, n).astype(np.uint8)))
    tracker.log_world.copy_(torch.from_numpy(rng.permutation(n).astype(np.int64)))
    tracker.finished.fill_(1)
    tracker._counts[0] = n
    return es, tracker


class TorchComposition(object):
    """the same steps with torch on the device (see the module docstring for what differs)"""

    def __init__(self, es, tracker):
        self.es, self.tracker = es, tracker
        P, H = es.networks, es.pairs
        self.theta = es.theta.clone()
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.t = 0
        self.perm = es.perm.long()
        self.blob = torch.zeros((P, es.blob_floats), dtype=torch.float32, device=DEV)
        self.eps = torch.zeros((max(H, 1), PARAMS), dtype=torch.float32, device=DEV)
        self.rows = torch.zeros((P, PARAMS), dtype=torch.float32, device=DEV)
        self.fitness = torch.zeros(P, dtype=torch.float32, device=DEV)

    def ask(self):
        es, H = self.es, self.es.pairs
        torch.randn(self.eps.shape, out=self.eps)
        d = es.sigma * self.eps
        self.rows[0:2 * H:2] = self.theta + d
        self.rows[1:2 * H:2] = self.theta - d
        if es.networks % 2:
            self.rows[2 * H] = self.theta
        self.blob.index_copy_(1, self.perm, self.rows)

    def score(self):
        tr, es = self.tracker, self.es
        p = torch.div(tr.log_world, es.seg, rounding_mode="floor")
        total = torch.zeros(es.networks, dtype=torch.float64, device=DEV).index_add_(0, p, tr.log_ret.double())
        count = torch.zeros(es.networks, dtype=torch.float64, device=DEV).index_add_(0, p, torch.ones_like(tr.log_ret, dtype=torch.float64))
        self.fitness.copy_(torch.where(count > 0, total / count, torch.full_like(total, -float("inf"))))

    def tell(self):
        es, H = self.es, self.es.pairs
        rank = torch.argsort(torch.argsort(self.fitness[:2 * H])).float()
        w = rank[0::2] - rank[1::2]
        ghat = (w @ self.eps) / (2.0 * H * (2 * H - 1) * es.sigma)
        grad = es.weight_decay * self.theta - ghat
        self.t += 1
        b1, b2 = es.betas
        self.m.mul_(b1).add_(grad, alpha=1 - b1)
        self.v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        self.theta.sub_(es.lr * (self.m / (1 - b1 ** self.t)) / ((self.v / (1 - b2 ** self.t)).sqrt() + es.eps))


def bench_calls(P, seg, calls, count):
    es, tracker = population(P, seg)
    es._warm_up(tracker)
    other = TorchComposition(es, tracker)
    es.fitness(tracker)
    other.score()
    torch.cuda.synchronize()
    # the two scores are the same means up to the fixed point and float32
    assert torch.allclose(es.fitness_out, other.fitness, rtol=1e-5, atol=1e-4), (es.fitness_out[:4], other.fitness[:4])
    steps = {"ask": (es.ask, other.ask), "fitness": (lambda: es.fitness(tracker), other.score), "tell": (es.tell, other.tell)}
    for what, (ours, theirs) in steps.items():
        for mode in ("eager", "graph"):
            variants = {"evo": ours, "torch": theirs}
            keep = []
            if mode == "graph":
                for name, fn in list(variants.items()):
                    try:
                        variants[name], g = captured(fn)
                        keep.append(g)
                    except Exception as e:                       # a baseline that cannot be captured is reported, not timed
                        emit(what=what, mode=mode, P=P, seg=seg, variant=name, error=str(e).splitlines()[0])
                        del variants[name]
            med, raw = windows(variants, calls, count)
            emit(what=what, mode=mode, P=P, seg=seg, calls=calls, windows=count, evo_us=med.get("evo"), torch_us=med.get("torch"), raw=raw)
    report = es.report()
    emit(what="state", P=P, seg=seg, generation=report["generation"], tells=report["tells"], t=report["t"],
         theta_finite=bool(torch.isfinite(es.theta).all()))


def bench_generation(P, seg, repeats):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.evolution import EvolutionStrategy
    from aquaticgymenv_amd.qbank import QNetworkBank
    base = [B.random_layers(100 + p) for p in range(min(P, 8))]
    bank = QNetworkBank([base[p % len(base)] for p in range(P)], seg, DEV)
    es = EvolutionStrategy(bank, sigma=0.05, lr=0.01, seed=3)
    env = BatchedAqua(P * seg, obstacles=False, seed=3, auto_reset=False, device=DEV)
    es.generation(env)                                          # untimed: the tracker, the kernels
    torch.cuda.synchronize()
    times, steps = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        es.generation(env)
        torch.cuda.synchronize()
        times.append(1000.0 * (time.perf_counter() - t0))
        steps.append(es.tracker.counts()["steps"])
    emit(what="generation", P=P, seg=seg, worlds=P * seg, repeats=repeats, ms=statistics.median(times), raw_ms=times, world_steps=steps,
         episodes=es.tracker.counts()["episodes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shapes", default="17x1024,257x64,4095x16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-generation", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: evolution strategies have no CPU path")
    emit(what="device", name=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip)
    for shape in filter(None, args.shapes.split(",")):
        P, seg = (int(v) for v in shape.split("x"))
        bench_calls(P, seg, args.calls, args.windows)
        if not args.no_generation:
            bench_generation(P, seg, args.repeats)


if __name__ == "__main__":
    main()
