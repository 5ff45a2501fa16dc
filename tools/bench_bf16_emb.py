#!/usr/bin/env python3
"""Rates of the bfloat16 embedding kernels beside the fp32 kernels, same process, same GPU, same inputs.

    python tools/bench_bf16_emb.py [--shape criteo_terabyte|mlperf_v2_multihot|both] [--repeats 20] [--warmup 3] [--scale 1.0] [--out FILE.md]

Shapes (bench.py WORKLOADS, as tools/bench_quant_emb.py takes them): Criteo-Terabyte (26 tables, D = 128, B = 65536, one lookup per bag,
int64 ids) and the multi-hot shape of BASELINE configs[4] (MLPerf-v2 tables, 214 lookups per sample, int32 ids).  Kernels, fp32 beside
bf16 tables holding the same values rounded to nearest:
  lookup   dlrm_emb_fwd                          | dlrm_emb_fwd_bf16
  SGD      dlrm_emb_bwd_sgd (DLRM_UPD_SORTED)    | dlrm_emb_bwd_sgd_bf16, nearest and stochastic rounding
  Adagrad  dlrm_emb_bwd_rowwise_adagrad          | dlrm_emb_bwd_rowwise_adagrad_bf16, nearest and stochastic rounding

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each kernel once between two HIP events (the
kernels alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported, with min / max.  The update kernels
include their sort.  Row bytes = what the kernel must move of the tables: one row read per lookup (lookup), one read + one write per
lookup (updates; an upper bound where rows repeat).  A measurement path that finds no GPU fails.  --scale < 1 shrinks every table
(rehearsals only: the output then says so)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def time_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_shape(name, wl, args, dev, lines):
    from dlrm_amd import ops
    D, B = wl["D"], wl["batch"]
    rows = [max(int(n * args.scale), 3) for n in wl["rows"]]
    hot = wl.get("hot") or [1] * len(rows)
    T = len(rows)
    idt = torch.int32 if wl.get("hot") else torch.int64
    isz = 4 if idt == torch.int32 else 8
    g = torch.Generator(device=dev).manual_seed(7)
    f32, b16 = [], []
    for n in rows:
        bound = float(np.sqrt(1.0 / n))
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-bound, bound, generator=g)
        f32.append(w)
        b16.append(w.to(torch.bfloat16))
    st32 = [torch.zeros(n, dtype=torch.float32, device=dev) for n in rows]
    st16 = [torch.zeros(n, dtype=torch.float32, device=dev) for n in rows]
    offs = [torch.arange(B, device=dev, dtype=idt) * h for h in hot]
    idxs = [torch.randint(0, n, (B * h,), device=dev, generator=g).to(idt) for n, h in zip(rows, hot)]
    bags = ops.BagBatch(offs, idxs)
    out = torch.empty((B, T * D), dtype=torch.float32, device=dev)
    dout = torch.empty((B, T * D), dtype=torch.float32, device=dev).uniform_(-1e-3, 1e-3, generator=g)
    lr, eps = 1e-3, 1e-8
    seed = [0]

    def next_seed():
        seed[0] += 1
        return seed[0]

    groups = {
        "lookup": {
            "dlrm_emb_fwd (fp32)": lambda: ops.emb_fwd(f32, bags, out),
            "dlrm_emb_fwd_bf16": lambda: ops.emb_fwd_bf16(b16, bags, out),
        },
        "SGD update": {
            "dlrm_emb_bwd_sgd sorted (fp32)": lambda: ops.emb_bwd_sgd(f32, bags, dout, lr, ops.UPD_SORTED),
            "dlrm_emb_bwd_sgd_bf16 nearest": lambda: ops.emb_bwd_sgd_bf16(b16, bags, dout, lr, "nearest", 0),
            "dlrm_emb_bwd_sgd_bf16 stochastic": lambda: ops.emb_bwd_sgd_bf16(b16, bags, dout, lr, "stochastic", next_seed()),
        },
        "row-wise Adagrad update": {
            "dlrm_emb_bwd_rowwise_adagrad (fp32)": lambda: ops.emb_bwd_rowwise_adagrad(f32, st32, bags, dout, lr, eps),
            "dlrm_emb_bwd_rowwise_adagrad_bf16 nearest": lambda: ops.emb_bwd_rowwise_adagrad_bf16(b16, st16, bags, dout, lr, eps, "nearest", 0),
            "dlrm_emb_bwd_rowwise_adagrad_bf16 stochastic": lambda: ops.emb_bwd_rowwise_adagrad_bf16(b16, st16, bags, dout, lr, eps, "stochastic", next_seed()),
        },
    }
    kernels = {k: fn for grp in groups.values() for k, fn in grp.items()}
    for _ in range(args.warmup):
        for fn in kernels.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in kernels}
    for _ in range(args.repeats):
        for k, fn in kernels.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    nnz = sum(B * h for h in hot)
    buf_bytes = B * T * D * 4                      # the pooled output (lookup) or the gradient buffer (updates: every lookup reads its bag's row of it)
    idx_bytes = nnz * isz + B * T * isz
    lines.append("")
    lines.append("### %s: %d tables, D = %d, B = %d, %d lookups per sample, %s ids, %.1f GB of fp32 tables%s" %
                 (name, T, D, B, sum(hot), "int32" if isz == 4 else "int64", sum(rows) * D * 4 / 1e9,
                  "" if args.scale == 1.0 else " — TABLES SCALED BY %g (rehearsal)" % args.scale))
    for gname, grp in groups.items():
        lines.append("")
        lines.append("| %s | median ms | min | max | table row MB | algorithmic GB/s | vs fp32 |" % gname)
        lines.append("|---|---|---|---|---|---|---|")
        base = None
        for k in grp:
            med = statistics.median(times[k])
            base = med if base is None else base
            elem = 2 if "bf16" in k else 4
            passes = 1 if gname == "lookup" else 2
            rb = nnz * D * elem * passes
            grad = 0 if gname == "lookup" else nnz * D * 4
            total = idx_bytes + rb + (buf_bytes if gname == "lookup" else grad)
            lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.0f | %.2fx |" %
                         (k, med, min(times[k]), max(times[k]), rb / 1e6, total / med / 1e6, base / med))
    del f32, b16, st32, st16, kernels, groups, bags
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["criteo_terabyte", "mlperf_v2_multihot", "both"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_bf16_emb.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup)]
    for name in (["criteo_terabyte", "mlperf_v2_multihot"] if args.shape == "both" else [args.shape]):
        run_shape(name, bench.WORKLOADS[name], args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
