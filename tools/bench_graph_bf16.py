#!/usr/bin/env python3
"""Step time of a bfloat16-table model at Criteo-Kaggle shapes, eager beside the whole-step HIP graph, same process, same GPU, same batches.

    python tools/bench_graph_bf16.py [--steps 200] [--warmup 20] [--rounds 5] [--timeout 300] [--row-cap 0] [--out FILE.md]

(profiles/graph_bf16/step_rates.md is `--out` of one run with the defaults.)

Three configurations (bench.py WORKLOADS["criteo_kaggle"]: 26 tables, D = 16, B = 2048, one lookup per bag, FusedSGD):
  eager bf16    the reference loop body on a model with bfloat16 tables, stochastic rounding (keys drawn on the host)
  graphed bf16  GraphedTrainStep(model, optimizer, device_step_state=True) on a twin of that model (keys drawn on the device)
  graphed fp32  GraphedTrainStep(model, optimizer) on the fp32 model: the configuration of the README's 0.320 ms

Protocol: every configuration is warmed up (the graphed ones through warm-up calls, capture and first replays), then `rounds` rounds; a round
times `steps` consecutive steps of each configuration in turn with a host clock around work that ends in a device synchronise (the
configurations alternate, so drift hits all alike); the MEDIAN ms / step over the rounds is reported, with min / max.  The kernel count of
a captured step is taken afterwards from a profiler trace of one replay (tracing slows the host: never inside a timed window).
The measurement runs in a child process under --timeout seconds; a run that finds no GPU fails.  --row-cap shrinks the tables
(rehearsals only: the output then says so)."""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(wl, rows, device, bf16):
    import numpy as np
    import torch
    import dlrm_amd
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedSGD
    D, nf = wl["D"], len(rows) + 1
    ln_top = np.asarray([D + nf * (nf - 1) // 2] + wl["top"])
    np.random.seed(123)
    torch.manual_seed(123)
    model = dlrm_amd.DLRM_Net(D, np.asarray(rows), np.asarray(wl["bot"]), ln_top, "dot", sigmoid_top=ln_top.size - 2,
                              loss_function="bce").to(device)
    model.emb_update_mode = ops.UPD_SORTED
    if bf16:
        model.embedding_bfloat16("stochastic", 2024)
    return model, FusedSGD(model.parameters(), lr=0.01)


def kernels_of_one_replay(call):
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


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_graph_bf16.py measures on the GPU; none found")
    import bench
    from dlrm_amd.graph import GraphedTrainStep
    device = torch.device("cuda:0")
    wl = bench.WORKLOADS["criteo_kaggle"]
    rows = [min(n, args.row_cap) if args.row_cap else n for n in wl["rows"]]
    B = wl["batch"]
    batches = bench.make_batches(8, B, rows, device, seed=5)

    me, oe = build(wl, rows, device, True)
    mg, og = build(wl, rows, device, True)
    mf, of = build(wl, rows, device, False)
    gb = GraphedTrainStep(mg, og, device_step_state=True)
    gf = GraphedTrainStep(mf, of)
    me.overlap_streams, me.update_in_backward = mg.overlap_streams, mg.update_in_backward

    def eager(i):
        X, off, idx, T = batches[i % len(batches)]
        oe.zero_grad()
        E = me.loss_fn(me(X, off, idx), T)
        E.backward()
        oe.step()
        return E.detach()

    configs = {"eager bf16": eager,
               "graphed bf16": lambda i: gb(*batches[i % len(batches)]),
               "graphed fp32": lambda i: gf(*batches[i % len(batches)])}
    for fn in configs.values():
        for i in range(max(args.warmup, 4)):
            fn(i)
        torch.cuda.synchronize()
    times = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = fn(i)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
            del loss
    assert gb.captures == 1 and gf.captures == 1, (gb.captures, gf.captures)
    og.state_dict()                                          # (settles the host mirrors: one key per step, warm-up included)
    calls = mg._bf16_update_calls
    counts = {"graphed bf16": kernels_of_one_replay(lambda: gb(*batches[0])), "graphed fp32": kernels_of_one_replay(lambda: gf(*batches[0]))}

    lines = ["GPU: %s; torch %s; Criteo-Kaggle shapes (26 tables%s, D = %d, B = %d, one lookup per bag, FusedSGD, sorted update)" %
             (torch.cuda.get_device_name(0), torch.__version__, "" if not args.row_cap else ", ROWS CAPPED AT %d (rehearsal)" % args.row_cap,
              wl["D"], B),
             "%d rounds of %d steps per configuration after %d warm-up steps, host clock around a device synchronise, median over the rounds" %
             (args.rounds, args.steps, max(args.warmup, 4)), "",
             "| step | median ms | min | max | vs eager bf16 | kernels in the captured step |", "|---|---|---|---|---|---|"]
    base = statistics.median(times["eager bf16"])
    for k in configs:
        med = statistics.median(times[k])
        lines.append("| %s | %.4f | %.4f | %.4f | %.2fx | %s |" % (k, med, min(times[k]), max(times[k]), base / med,
                                                                  "-" if k not in counts else counts[k] if counts[k] else "not measured"))
    lines += ["", "graphed bf16: one capture, %d update calls counted on the device and mirrored on the host; embedding update of the fp32 graph: %s" %
              (calls, {0: "atomic", 1: "deterministic", 2: "sorted"}.get(int(mf.emb_update_mode), "?"))]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring child process may take")
    ap.add_argument("--row-cap", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the run itself: a fresh child process under a time limit (this parent never opens the GPU)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=args.timeout)
    except subprocess.TimeoutExpired:
        sys.exit("ERROR: tools/bench_graph_bf16.py: the measurement did not finish in %d s" % args.timeout)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
