#!/usr/bin/env python3
"""Small-batch forward latency, eager beside dlrm_amd.graph.GraphedForward, one process, same GPU, same requests.

    python tools/bench_graph_forward.py [--min-seconds 0.5] [--repeats 3] [--row-cap 500000] [--timeout 900] [--only kaggle|terabyte]
                                        [--out FILE.md]

(profiles/graph_forward/rates.md is `--out` of one run with the defaults.)

Cells.  Criteo-Kaggle shapes (bench.py WORKLOADS["criteo_kaggle"]: 26 tables, D = 16) at B = 64, 256, 2048, list inputs (53 tensors per
request) and stacked [T, B] inputs, three models: fp32; 8-bit tables with fp16 towers; 8-bit tables with int8 towers.  Criteo-Terabyte
widths (D = 128) at B = 2048 for fp32 and 8-bit tables.  The graphed forward runs with batch_sizes = (64, 256, 2048) except for the int8
towers, which quantise per batch and therefore take exact-shape graphs.  For list inputs a third column replays with the staging kernel
turned off (one hipMemcpyAsync per tensor): the A/B behind graph_forward.STAGE_MEMCPY_MAX.

Protocol.  Every cell is warmed up (the graphed one through its eager calls, capture and first replays), then `repeats` times: eager, graphed
(and graphed with copies) in turn, each timed for at least `min-seconds` of back-to-back calls with a host clock around work that ends in a
device synchronise.  Reported: median ms per request over the repeats with min / max.  "slower": the graphed median is above the eager
median by more than the larger of the two cells' (max - min).  Requests cycle through 8 batches per cell, so the offsets proof of a request
is paid once per tensor object on both sides (a server that builds new offsets tensors per request pays it per request unless their
producer tags them: dlrm_amd.ops.mark_one_lookup_per_bag).  Kernel counts come from a profiler trace of one replay, outside the timed windows.
The measurement runs in a child process under --timeout seconds; a run that finds no GPU fails.  --row-cap caps the tables' row counts as
bench.py --row-cap does (0: full size)."""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUCKETS = (64, 256, 2048)
MODELS = {"fp32": (0, 32), "q8 tables + fp16 towers": (8, 16), "q8 tables + int8 towers": (8, 8), "q8 tables": (8, 32)}


def build(wl, rows, device, emb_bits, mlp_bits):
    import numpy as np
    import torch
    import dlrm_amd
    D, nf = wl["D"], len(rows) + 1
    ln_top = np.asarray([D + nf * (nf - 1) // 2] + wl["top"])
    np.random.seed(123)
    torch.manual_seed(123)
    model = dlrm_amd.DLRM_Net(D, np.asarray(rows), np.asarray(wl["bot"]), ln_top, "dot", sigmoid_top=ln_top.size - 2,
                              loss_function="bce").to(device)
    if emb_bits:
        model.quantize_embedding(emb_bits)
    if mlp_bits != 32:
        model.quantize_mlp(mlp_bits)
    return model


def kernels_of_one_call(call):
    """device kernels one call launches, from a profiler trace (None: the profiler reported none)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:                                   # noqa: BLE001 - the count is a diagnostic
        print("profiler: %s: %s" % (type(e).__name__, e), file=sys.stderr)
        return None


def timed(fn, min_s):
    """ms per call over at least min_s of back-to-back calls, a device synchronise inside the window"""
    import torch
    torch.cuda.synchronize()
    t0, k = time.perf_counter(), 0
    while True:
        for _ in range(20):
            fn(k)
            k += 1
        if time.perf_counter() - t0 >= min_s:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_graph_forward.py measures on the GPU; none found")
    import bench
    from dlrm_amd import graph_forward
    from dlrm_amd.graph import GraphedForward
    device = torch.device("cuda:0")
    plan = []
    if args.only in (None, "kaggle"):
        plan.append(("criteo_kaggle", ("fp32", "q8 tables + fp16 towers", "q8 tables + int8 towers"), (64, 256, 2048)))
    if args.only in (None, "terabyte"):
        plan.append(("criteo_terabyte", ("fp32", "q8 tables"), (2048,)))
    rows_out, any_slower, ab = [], [], []
    for wl_name, models, sizes in plan:
        wl = bench.WORKLOADS[wl_name]
        rows = [min(n, args.row_cap) if args.row_cap else n for n in wl["rows"]]
        stacked = {B: bench.make_batches(8, B, rows, device, seed=5) for B in sizes}
        for mname in models:
            emb_bits, mlp_bits = MODELS[mname]
            model = build(wl, rows, device, emb_bits, mlp_bits)
            buckets = None if mlp_bits == 8 else BUCKETS
            for B in sizes:
                for structure in ("list", "stacked"):
                    if structure == "stacked":
                        reqs = [(X, o, i) for X, o, i, _ in stacked[B]]
                    else:
                        reqs = [(X, list(o.unbind(0)), list(i.unbind(0))) for X, o, i, _ in stacked[B]]
                    fwd = GraphedForward(model, batch_sizes=buckets)
                    fns = {"eager": lambda k, r=reqs: model(*r[k % len(r)])}
                    fns["graphed"] = lambda k, r=reqs, f=fwd: f(*r[k % len(r)])
                    if structure == "list":
                        fcp = GraphedForward(model, batch_sizes=buckets)
                        fcp.stage_memcpy_max = 1 << 30
                        fns["graphed, copies"] = lambda k, r=reqs, f=fcp: f(*r[k % len(r)])
                    with torch.no_grad():
                        for fn in fns.values():
                            for k in range(2 * len(reqs) + 4):
                                fn(k)
                            torch.cuda.synchronize()
                        t = {name: [] for name in fns}
                        for _ in range(args.repeats):
                            for name, fn in fns.items():
                                t[name].append(timed(fn, args.min_seconds))
                        nk = kernels_of_one_call(lambda: fns["graphed"](0))
                    assert fwd.captures == 1, fwd.captures
                    med = {name: statistics.median(v) for name, v in t.items()}
                    spread = max(max(t["eager"]) - min(t["eager"]), max(t["graphed"]) - min(t["graphed"]))
                    slower = med["graphed"] > med["eager"] + spread
                    cell = "%s D = %d, %s, B = %d, %s" % (wl_name, wl["D"], mname, B, structure)
                    if slower:
                        any_slower.append(cell)
                    fmt = lambda v: "%.4f (%.4f - %.4f)" % (statistics.median(v), min(v), max(v))      # noqa: E731
                    rows_out.append("| %s | %d | %s | %s | %s | %s | %s | %.2fx | %s | %s | %s |" % (
                        wl_name.replace("criteo_", ""), wl["D"], mname, B, structure, fmt(t["eager"]), fmt(t["graphed"]),
                        med["eager"] / med["graphed"], "SLOWER" if slower else "no", "buckets" if buckets else "exact",
                        nk if nk else "not measured"))
                    if structure == "list":
                        segments = (list(fwd._buckets.values()) + fwd._exact.values())[0].plan.n
                        ab.append("| %s | %d | %s | %d | %d | %s | %s |" % (wl_name.replace("criteo_", ""), wl["D"], mname, B, segments,
                                                                            fmt(t["graphed"]), fmt(t["graphed, copies"])))
                    del fwd, fns
            del model
            torch.cuda.empty_cache()
    lines = ["GPU: %s; torch %s; tables %s" % (torch.cuda.get_device_name(0), torch.__version__,
                                              "at full size" if not args.row_cap else "capped at %d rows" % args.row_cap),
             "%d repeats per cell, each at least %.2f s of back-to-back requests per configuration (eager, graphed in turn), host clock around a "
             "device synchronise; ms per request: median (min - max)" % (args.repeats, args.min_seconds),
             "staging threshold in this run: graph_forward.STAGE_MEMCPY_MAX = %d" % graph_forward.STAGE_MEMCPY_MAX, "",
             "| shapes | D | model | B | inputs | eager ms | graphed ms | eager / graphed | slower beyond the spread | graphs | kernels per replay |",
             "|---|---|---|---|---|---|---|---|---|---|---|"] + rows_out
    lines += ["", "Staging of list inputs: one dlrm_stage_inputs launch against one hipMemcpyAsync per segment (same graphs, same requests)", "",
              "| shapes | D | model | B | segments | graphed, staging kernel ms | graphed, copies ms |", "|---|---|---|---|---|---|---|"] + ab
    lines += ["", "cells where the graphed forward is slower than eager beyond the spread: %s" % ("; ".join(any_slower) if any_slower else "none")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--row-cap", type=int, default=500000)
    ap.add_argument("--only", choices=("kaggle", "terabyte"), default=None)
    ap.add_argument("--timeout", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the run itself: a fresh child process under a time limit (this parent never opens the GPU)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("ERROR: tools/bench_graph_forward.py: the measurement did not finish in %d s" % args.timeout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
