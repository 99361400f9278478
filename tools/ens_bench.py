#!/usr/bin/env python3
"""One ensemble launch (aquaens_act_f32) against the composition it replaces, on one GPU.

    python tools/ens_bench.py [--calls 200] [--windows 5] [--warmup 20] [--shapes 2x262144,16x16384,16x262144,256x1024]

For every shape (M member networks x N worlds, greedy, normalised [5][N] input) these do the same work on the same weights
and are checked to choose the same actions before anything is timed:

  ens_mean / ens_vote   one aquaens_act_f32 (actions out), mode mean / vote
  ens_stats             the same in mode mean with the variance and the votes written as well
  compose               what the launch replaces: the input tiled M times into a preallocated [5][M * N] tensor, one
                        aquabank_act_f32 with seg = N writing q [3][M * N], then the float64 mean over the members and the
                        arg-max in torch; `tile` is the tiling alone
  policy                aquapol_act_f32 alone on slot 0 and the same N worlds (tools/policy_bench.py's act_only leg), eagerly
                        and as a one-node graph; M x policy is what M policy launches cost when each is issued by itself.  At
                        small N that is the launch period, not kernel time
  m_policies_graph      the M policy launches, launch p on slot p, captured as ONE graph of M nodes: what the same MFMA work
                        costs the device when no host sits between the launches
  matrix_floor          no measurement: M x N x 9 216 FLOP over the 157.3 TFLOP/s float32 matrix peak, the least time the
                        member loop's matrix work can take on a full device

The ensemble variants are issued eagerly from Python through ctypes (`*_eager`) and replayed as one captured graph node
(`*_graph`).  A window is --calls calls between two HIP events; the variants alternate window by window, --windows windows
each; the figure is the MEDIAN window's microseconds per call.  Nothing here is a pass / fail threshold.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_WORLD = 2 * (5 * 64 + 64 * 64 + 64 * 3)
F32_MATRIX_PEAK_TF = 157.3


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
    ap.add_argument("--shapes", default="2x262144,16x16384,16x262144,256x1024")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("ens_bench.py measures on a GPU; none is visible")
    from aquaticgymenv_amd import _ens_capi
    from aquaticgymenv_amd.ensemble import QEnsemble
    from aquaticgymenv_amd.qbank import QNetworkBank

    dev = "cuda:0"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    trained = [[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for tag in ("no_obs", "with_obs")]
    result = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "calls_per_window": args.calls, "windows": args.windows,
              "warmup": args.warmup, "group": _ens_capi.GROUP, "unit": "us per call (median window)", "shapes": {}}
    for shape in args.shapes.split(","):
        M, n = (int(v) for v in shape.split("x"))
        rng = np.random.RandomState(M)
        # the two trained networks, then perturbed copies of them: M different slots
        nets = [[(k + (0.01 * rng.randn(*k.shape)).astype(np.float32) * (p >= 2), b) for k, b in trained[p % 2]] for p in range(M)]
        bank = QNetworkBank(nets, n, dev)                    # seg = N: what the composition needs
        buf = torch.rand((5, n), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        ens = {mode: QEnsemble(bank, mode=mode) for mode in ("mean", "vote")}
        stats = QEnsemble(bank, mode="mean").attach(variance=torch.zeros((3, n), dtype=torch.float32, device=dev),
                                                     votes=torch.zeros((3, n), dtype=torch.int32, device=dev))
        out = {name: torch.zeros(n, dtype=torch.uint8, device=dev) for name in ("mean", "vote", "stats", "policy")}
        tiled = torch.zeros((5, M * n), dtype=torch.float32, device=dev)
        q_all = torch.zeros((3, M * n), dtype=torch.float32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        in_ptr = buf.data_ptr()

        def run_ens(name, policy, s=stream):
            rc = policy.launch(in_ptr, n, True, n, 0, 0.0, 0, 0, None, out[name].data_ptr(), None, 0, None, s)
            assert rc == 0, policy.last_error

        def tile():
            tiled.view(5, M, n).copy_(buf.unsqueeze(1).expand(5, M, n))

        def compose():
            tile()
            bank.q_values(tiled, out=q_all)
            return q_all.view(3, M, n).double().mean(dim=1).float().argmax(dim=0)

        views = [bank.view(p) for p in range(M)]

        def policy():
            views[0].act(buf, out=out["policy"])

        def m_policies():
            for v in views:
                v.act(buf, out=out["policy"])

        for name in ("mean", "vote"):
            run_ens(name, ens[name])
        run_ens("stats", stats)
        composed = compose()
        torch.cuda.synchronize()
        assert torch.equal(out["mean"], out["stats"]) and torch.equal(out["mean"].long(), composed), "the variants disagree"

        graphs = {}
        for name, pol in (("mean", ens["mean"]), ("vote", ens["vote"]), ("stats", stats)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run_ens(name, pol, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            graphs[name] = g
        for name, fn in (("policy", policy), ("m_policies", m_policies)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[name] = g
        variants = [("ens_mean_eager", lambda: run_ens("mean", ens["mean"])), ("ens_vote_eager", lambda: run_ens("vote", ens["vote"])),
                    ("ens_stats_eager", lambda: run_ens("stats", stats)), ("ens_mean_graph", graphs["mean"].replay),
                    ("ens_vote_graph", graphs["vote"].replay), ("ens_stats_graph", graphs["stats"].replay),
                    ("compose", compose), ("tile", tile), ("policy", policy), ("policy_graph", graphs["policy"].replay),
                    ("m_policies_graph", graphs["m_policies"].replay)]
        for _, fn in variants:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.windows):
            for name, fn in variants:                        # alternating: drift hits every variant alike
                times[name].append(window(torch, fn, args.calls))
        row = {"members": M, "worlds": n, "shape": list(_ens_capi.shape(n, cus))}
        for name, _ in variants:
            row[name] = round(statistics.median(times[name]), 3)
            row[name + "_windows"] = [round(v, 3) for v in times[name]]
        row["M_x_policy"] = round(M * row["policy"], 3)
        row["M_x_policy_graph"] = round(M * row["policy_graph"], 3)
        row["matrix_floor"] = round(M * n * FLOP_PER_WORLD / (F32_MATRIX_PEAK_TF * 1e6), 3)
        row["ens_mean_graph_over_m_policies_graph"] = round(row["ens_mean_graph"] / row["m_policies_graph"], 2)
        row["ens_mean_graph_over_matrix_floor"] = round(row["ens_mean_graph"] / row["matrix_floor"], 2)
        row["compose_over_ens_mean_eager"] = round(row["compose"] / row["ens_mean_eager"], 2)
        row["ens_mean_graph_tflops"] = round(M * n * FLOP_PER_WORLD / row["ens_mean_graph"] * 1e-6, 2)
        result["shapes"][shape] = row
        del bank, tiled, q_all
    print(json.dumps(result))


if __name__ == "__main__":
    main()
