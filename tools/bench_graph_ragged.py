#!/usr/bin/env python3
"""Ragged multi-hot requests: the eager forward beside dlrm_amd.graph.GraphedForward without and with ragged buckets (lookup_capacity),
one process, same GPU, same requests.

    python tools/bench_graph_ragged.py [--min-seconds 0.5] [--repeats 3] [--row-cap 500000] [--timeout 900] [--out FILE.md]

(profiles/graph_forward/ragged_rates.md is `--out` of one run with the defaults.)

Cells.  Criteo-Kaggle shapes (bench.py WORKLOADS["criteo_kaggle"]: 26 tables, D = 16, fp32) at B = 64, 256, 2048, list inputs; every bag
draws its own size, uniform in 1 .. P, for P = 4 and 10 (the reference's --num-indices-per-lookup-fixed False).  Requests cycle through 8
different batches per cell, so every request has its own nnz per table.  Columns:
    eager        model(X, lS_o, lS_i)
    exact        GraphedForward(batch_sizes=(64, 256, 2048)): no lookup_capacity, every shape tuple an exact-shape graph of its own.  The 8
                 batches of a cell just FIT its LRU of 8 graphs, the best case of this form; `exact, 16 shapes` cycles through 16 batches
                 instead, more shapes than the LRU holds — what a stream of new shapes does to it
    ragged       the same with lookup_capacity=P: one ragged bucket per batch size
Recorded beside the times: captures per 100 requests inside the timed windows, and staging launches per replay.

Protocol.  As tools/bench_graph_forward.py: every configuration is warmed up, then `repeats` times each configuration in turn is timed for
at least `min-seconds` of back-to-back calls with a host clock around work that ends in a device synchronise; median ms per request with
min / max.  "slower": a median above the other's by more than the larger of the two (max - min).  The measurement runs in a child process
under --timeout seconds; a run that finds no GPU fails."""
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
BAG_SIZES = (4, 10)


def build(wl, rows, device):
    import numpy as np
    import torch
    import dlrm_amd
    D, nf = wl["D"], len(rows) + 1
    ln_top = np.asarray([D + nf * (nf - 1) // 2] + wl["top"])
    np.random.seed(123)
    torch.manual_seed(123)
    return dlrm_amd.DLRM_Net(D, np.asarray(rows), np.asarray(wl["bot"]), ln_top, "dot", sigmoid_top=ln_top.size - 2,
                             loss_function="bce").to(device)


def ragged_batches(count, B, P, rows, m_den, device, seed):
    """`count` requests of B rows: every bag of every table draws its own size in 1 .. P"""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        X = torch.rand((B, m_den), generator=g).to(device)
        offs, ids = [], []
        for r in rows:
            lens = torch.randint(1, P + 1, (B,), generator=g)
            offs.append((torch.cumsum(lens, 0) - lens).to(device))
            ids.append(torch.randint(0, r, (int(lens.sum()),), generator=g).to(device))
        out.append((X, offs, ids))
    return out


def timed(fn, min_s):
    """(ms per call, calls) over at least min_s of back-to-back calls, a device synchronise inside the window"""
    import torch
    torch.cuda.synchronize()
    t0, k = time.perf_counter(), 0
    while True:
        for _ in range(16):
            fn(k)
            k += 1
        if time.perf_counter() - t0 >= min_s:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3, k


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_graph_ragged.py measures on the GPU; none found")
    import bench
    from dlrm_amd.graph import GraphedForward
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["criteo_kaggle"]
    rows = [min(n, args.row_cap) if args.row_cap else n for n in wl["rows"]]
    model = build(wl, rows, device)
    m_den = int(wl["bot"][0])
    table, notes_eager, notes_exact = [], [], []
    fmt = lambda v: "%.4f (%.4f - %.4f)" % (statistics.median(v), min(v), max(v))      # noqa: E731
    for B in BUCKETS:
        for P in BAG_SIZES:
            reqs = ragged_batches(16, B, P, rows, m_den, device, seed=1000 * P + B)
            r8 = reqs[:8]
            assert len({tuple(i.numel() for i in r[2]) for r in reqs}) == len(reqs)
            fwds = {"exact": GraphedForward(model, batch_sizes=BUCKETS), "exact, 16 shapes": GraphedForward(model, batch_sizes=BUCKETS),
                    "ragged": GraphedForward(model, batch_sizes=BUCKETS, lookup_capacity=P)}
            fns = {"eager": lambda k, r=r8: model(*r[k % len(r)])}
            for name, f in fwds.items():
                fns[name] = lambda k, r=(reqs if "16" in name else r8), f=f: f(*r[k % len(r)])
            t = {name: [] for name in fns}
            calls = {name: 0 for name in fwds}
            with torch.no_grad():
                for fn in fns.values():
                    for k in range(3 * 16 + 4):
                        fn(k)
                    torch.cuda.synchronize()
                before = {name: (f.captures, f.replays, f.staged_launches) for name, f in fwds.items()}
                for _ in range(args.repeats):
                    for name, fn in fns.items():
                        ms, k = timed(fn, args.min_seconds)
                        t[name].append(ms)
                        if name in calls:
                            calls[name] += k
            med = {name: statistics.median(v) for name, v in t.items()}
            spread = lambda a, b: max(max(t[a]) - min(t[a]), max(t[b]) - min(t[b]))     # noqa: E731
            caps, per = {}, {}
            for name, f in fwds.items():
                c0, r0, s0 = before[name]
                caps[name] = 100.0 * (f.captures - c0) / max(calls[name], 1)
                per[name] = (f.staged_launches - s0) / max(f.replays - r0, 1)
            cell = "B = %d, P = %d" % (B, P)
            if med["ragged"] > med["eager"] + spread("ragged", "eager"):
                notes_eager.append(cell)
            if med["ragged"] > med["exact"] + spread("ragged", "exact"):
                notes_exact.append(cell)
            rg = fwds["ragged"]
            assert rg.captures == 1 and rg.ragged_buckets_in_use == 1 and rg.exact_shapes == 0, (rg.captures, rg.exact_shapes)
            mean_nnz = sum(i.numel() for r in r8 for i in r[2]) / (8.0 * len(rows))
            table.append("| %d | %d | %.0f / %d | %s | %s | %s | %s | %.2fx | %.2fx | %.2fx | %.1f / %.1f / %.1f | %.2f / %.2f |" % (
                B, P, mean_nnz, B * P, fmt(t["eager"]), fmt(t["exact"]), fmt(t["exact, 16 shapes"]), fmt(t["ragged"]),
                med["eager"] / med["ragged"], med["exact"] / med["ragged"], med["exact, 16 shapes"] / med["ragged"],
                caps["exact"], caps["exact, 16 shapes"], caps["ragged"], per["exact"], per["ragged"]))
            del fwds, fns
            torch.cuda.empty_cache()
    lines = ["GPU: %s; torch %s; Criteo-Kaggle shapes (26 tables, D = 16, fp32), tables %s; list inputs, bag sizes uniform in 1 .. P"
             % (torch.cuda.get_device_name(0), torch.__version__, "at full size" if not args.row_cap else "capped at %d rows" % args.row_cap),
             "command: python tools/bench_graph_ragged.py " + " ".join(a for a in sys.argv[1:] if a != "--child"),
             "%d repeats per cell, each at least %.2f s of back-to-back requests per configuration in turn, host clock around a device "
             "synchronise; ms per request: median (min - max).  exact: GraphedForward(batch_sizes) over 8 shapes (they fit its LRU of 8); "
             "exact, 16 shapes: the same over 16 shapes; ragged: lookup_capacity = P" % (args.repeats, args.min_seconds), "",
             "| B | P | mean nnz per table / Lcap | eager ms | exact ms | exact, 16 shapes ms | ragged ms | eager / ragged | exact / ragged | "
             "exact 16 / ragged | captures per 100 requests (exact / exact 16 / ragged) | staging launches per replay (exact / ragged) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"] + table
    lines += ["", "cells where ragged buckets are slower than eager beyond the spread: %s" % ("; ".join(notes_eager) or "none"),
              "cells where ragged buckets are slower than exact-shape graphs over 8 shapes beyond the spread: %s" % ("; ".join(notes_exact) or "none")]
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
        sys.exit("ERROR: tools/bench_graph_ragged.py: the measurement did not finish in %d s" % args.timeout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
