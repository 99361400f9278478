#!/usr/bin/env python3
"""One bank launch (aquabank_act_f32) against the P launches of aquapol_act_f32 it replaces, on one GPU.

    python tools/bank_bench.py [--calls 200] [--windows 5] [--warmup 20] [--shapes 2x131072,150x1024,4096x16]

For every shape (P networks x seg worlds each, greedy, normalised [5][P * seg] input, actions out) two variants do the same
work on the same weights -- the bank's slots -- and are checked to write the same actions before anything is timed:

  bank      one aquabank_act_f32 over all P * seg worlds
  policy    P aquapol_act_f32, launch p on slot p and columns [p * seg, (p + 1) * seg)

each issued eagerly from Python through ctypes (`*_eager`) and replayed as one captured graph (`*_graph`: no host work per
launch, the device-side cost of P launch periods against one).  A window is --calls calls between two HIP events; the
variants alternate window by window, --windows windows each; the figure is the MEDIAN window's microseconds per call.
The comparison is against the existing kernel, never against the bank itself.  One JSON line.
"""
import argparse
import ctypes
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
    ap.add_argument("--shapes", default="2x131072,150x1024,4096x16")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bank_bench.py measures on a GPU; none is visible")
    from aquaticgymenv_amd import _policy_capi
    from aquaticgymenv_amd.qbank import QNetworkBank

    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    trained = [[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for tag in ("no_obs", "with_obs")]
    result = {"device": torch.cuda.get_device_name(0), "calls_per_window": args.calls, "windows": args.windows, "warmup": args.warmup,
              "unit": "us per call (median window)", "shapes": {}}
    for shape in args.shapes.split(","):
        P, seg = (int(v) for v in shape.split("x"))
        n = P * seg
        rng = np.random.RandomState(P)
        # the two trained networks, then perturbed copies of them: P different slots
        nets = [[(k + (0.01 * rng.randn(*k.shape)).astype(np.float32) * (p >= 2), b) for k, b in trained[p % 2]] for p in range(P)]
        bank = QNetworkBank(nets, seg, dev)
        buf = torch.rand((5, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        out_bank = torch.zeros(n, dtype=torch.uint8, device=dev)
        out_pol = torch.zeros(n, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        slot, in_ptr, pol_ptr, act = bank.tensor.stride(0), buf.data_ptr(), out_pol.data_ptr(), _policy_capi.lib.aquapol_act_f32
        base = bank.tensor.data_ptr()

        def run_bank(s=stream):
            rc = bank.launch(in_ptr, n, True, n, 0, 0.0, 0, 0, None, out_bank.data_ptr(), None, 0, None, s)
            assert rc == 0, bank.last_error

        def run_policy(s=stream):
            for p in range(P):
                rc = act(base + p * slot, in_ptr + 4 * p * seg, n, 1, seg, p * seg, 0.0, 0, 0, None, pol_ptr + p * seg, None, 0, None, s)
                assert rc == 0

        run_bank()
        run_policy()
        torch.cuda.synchronize()
        assert torch.equal(out_bank, out_pol), "the two variants disagree"

        graphs = {}
        for name, fn in (("bank", run_bank), ("policy", run_policy)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            graphs[name] = g
        variants = [("bank_eager", run_bank), ("policy_eager", run_policy), ("bank_graph", graphs["bank"].replay),
                    ("policy_graph", graphs["policy"].replay)]
        for _, fn in variants:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.windows):
            for name, fn in variants:                        # alternating: drift hits every variant alike
                times[name].append(window(torch, fn, args.calls))
        row = {"networks": P, "seg": seg, "worlds": n}
        for name, _ in variants:
            row[name] = round(statistics.median(times[name]), 3)
            row[name + "_windows"] = [round(v, 3) for v in times[name]]
        row["eager_policy_over_bank"] = round(row["policy_eager"] / row["bank_eager"], 2)
        row["graph_policy_over_bank"] = round(row["policy_graph"] / row["bank_graph"], 2)
        result["shapes"][shape] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
