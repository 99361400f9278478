#!/usr/bin/env python3
"""One Q-value map launch (aquaqmap_maps_f32) against the composition it replaces, on one GPU.

    python tools/qmap_bench.py [--calls 200] [--windows 5] [--warmup 20] [--shapes 1x1x100x8,2x1x100x8,256x1x100x8,16x16x100x8]

For every shape (P networks x G goals x a W x W world x S sectors, the reference's grid) two variants write the best action
and the best Q-value of every state from the same weights -- the bank's slots -- and are checked to write the same bits
before anything is timed:

  map       one aquaqmap_maps_f32: the inputs made in registers from the tables, 5 bytes written per state
  composed  QNetworkBank.q_values over a float32 [5][P * G * S * W * W] states tensor tiled per network and goal (20 bytes
            read and 12 written per state), then torch.max over the three Q-values and the cast of its indices to uint8.
            The states tensor is built once, outside the timed windows; `build_states_us` is the time of that build on the
            device (torch indexing and broadcast copies), which a caller pays again whenever the goals change.

each issued eagerly from Python (`*_eager`) and replayed as one captured graph (`*_graph`).  A window is --calls calls
between two HIP events; the variants alternate window by window, --windows windows each; the figure is the MEDIAN window's
microseconds per call.  `map_mfma_share` is the least time the matrix pipe needs for the map's tiles (70
v_mfma_f32_32x32x2_f32 of 64 cycles per tile of 32 states, on 4 SIMDs per compute unit at the device's clock) over the
graph time: a share of the bound, not a kernel trace.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(torch, call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", default="1x1x100x8,2x1x100x8,256x1x100x8,16x16x100x8")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("qmap_bench.py measures on a GPU; none is visible")
    from aquaticgymenv_amd import _qmap_capi
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qmaps import QValueMaps

    dev = "cuda:0"
    props = torch.cuda.get_device_properties(0)
    cus, mhz = props.multi_processor_count, getattr(props, "clock_rate", 2400000) / 1e3     # kHz; the MI355X's 2400 MHz where torch does not say
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    trained = [[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for tag in ("no_obs", "with_obs")]
    result = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "clock_mhz": mhz, "calls_per_window": args.calls,
              "windows": args.windows, "warmup": args.warmup, "unit": "us per call (median window)", "shapes": {}}
    for shape in args.shapes.split(","):
        P, G, W, S = (int(v) for v in shape.split("x"))
        M = S * W * W
        n = P * G * M
        rng = np.random.RandomState(P)
        # the two trained networks, then perturbed copies of them: P different slots
        nets = [[(k + (0.01 * rng.randn(*k.shape)).astype(np.float32) * (p >= 2), b) for k, b in trained[p % 2]] for p in range(P)]
        bank = QNetworkBank(nets, G * M, dev)                 # the composition's segment: network p takes its G maps
        maps = QValueMaps.reference(bank, W, S)
        goals = torch.as_tensor(QValueMaps.normalised_goals(rng.randint(1, W, size=(G, 2)), W), device=dev)
        m_action = torch.zeros((P, G, S, W, W), dtype=torch.uint8, device=dev)
        m_value = torch.zeros((P, G, S, W, W), dtype=torch.float32, device=dev)
        c_action, c_value = torch.zeros_like(m_action), torch.zeros_like(m_value)
        c_index = torch.zeros(n, dtype=torch.int64, device=dev)
        q = torch.zeros((3, n), dtype=torch.float32, device=dev)
        states = torch.zeros((5, P, G, M), dtype=torch.float32, device=dev)
        m = torch.arange(M, device=dev)
        c, r, k = m % W, (m // W) % W, m // (W * W)

        def build_states():
            states[0], states[1], states[2] = maps.xs[c], maps.ys[r], maps.angles[k]       # broadcast over [P, G]
            states[3], states[4] = goals[:, 0][None, :, None], goals[:, 1][None, :, None]

        flat = states.view(5, n)

        def run_map():
            maps.maps(goals, action=m_action, value=m_value)

        def run_composed():
            bank.q_values(flat, out=q)
            torch.max(q, dim=0, out=(c_value.view(n), c_index))
            c_action.view(n).copy_(c_index)

        build_states()
        run_map()
        run_composed()
        torch.cuda.synchronize()
        assert torch.equal(m_value.view(torch.int32), c_value.view(torch.int32)), "the two variants disagree on the values"
        # torch.max names an index of the maximum, not necessarily the lowest on an exact tie: compare where the maximum is unique
        unique = (q == c_value.view(1, n)).sum(dim=0) == 1
        assert torch.equal(m_action.view(n)[unique], c_action.view(n)[unique]), "the two variants disagree on the actions"
        build = sorted(window(torch, build_states, 3) for _ in range(args.windows))[args.windows // 2]

        graphs = {}
        for name, fn in (("map", run_map), ("composed", run_composed)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[name] = g
        variants = [("map_eager", run_map), ("composed_eager", run_composed), ("map_graph", graphs["map"].replay),
                    ("composed_graph", graphs["composed"].replay)]
        for _, fn in variants:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.windows):
            for name, fn in variants:                        # alternating: drift hits every variant alike
                times[name].append(window(torch, fn, args.calls))
        items = int(_qmap_capi.lib.aquaqmap_items(P, G, W, W, S))
        row = {"networks": P, "goals": G, "world": W, "sectors": S, "states": n, "items": items,
               "states_tensor_mb": round(20 * n / 1e6, 1), "build_states_us": round(build, 1)}
        for name, _ in variants:
            row[name] = round(statistics.median(times[name]), 3)
            row[name + "_windows"] = [round(v, 3) for v in times[name]]
        row["eager_composed_over_map"] = round(row["composed_eager"] / row["map_eager"], 2)
        row["graph_composed_over_map"] = round(row["composed_graph"] / row["map_graph"], 2)
        mfma_floor_us = items * 70 * 64 / (4 * cus) / mhz
        row["map_mfma_floor_us"] = round(mfma_floor_us, 3)
        row["map_mfma_share"] = round(mfma_floor_us / row["map_graph"], 3)
        result["shapes"][shape] = row
        del states, flat, q, c_index, graphs, bank, maps
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
