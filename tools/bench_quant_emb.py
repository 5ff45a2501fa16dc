#!/usr/bin/env python3
"""Lookup rates of the quantised embedding kernels beside the fp32 kernel, same process, same GPU, same inputs.

    python tools/bench_quant_emb.py [--shape criteo_terabyte|mlperf_v2_multihot|both] [--repeats 30] [--warmup 5] [--scale 1.0] [--out FILE.md]

Shapes (bench.py WORKLOADS, tables at full size): Criteo-Terabyte (26 tables, D = 128, B = 65536, one lookup per bag, int64 ids) and
the multi-hot shape of BASELINE configs[4] (MLPerf-v2 tables, 214 lookups per sample, int32 ids).  Kernels: dlrm_emb_fwd (fp32),
dlrm_emb_fwd_quant at 8 and 4 bits, and dlrm_emb_quantize_rows (the prepack, timed once per table set while it runs).

Protocol (docs/MEASUREMENT.md): warm-up launches, then `repeats` rounds; every round times each of the three lookup kernels once between
two HIP events (the kernels alternate inside a round, so drift hits all three alike); the MEDIAN over the rounds is reported, with min / max.
Algorithmic bytes = indices + offsets + row bytes of every lookup + the output, computed from the shapes; rate = bytes / median time.
A measurement path that finds no GPU fails.  --scale < 1 shrinks every table (rehearsals only: the output then says so)."""
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
    tables = []
    for n in rows:
        bound = float(np.sqrt(1.0 / n))
        tables.append(torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-bound, bound, generator=g))
    torch.cuda.synchronize()
    packed, pack_ms = {}, {}
    for bits in (8, 4):
        ops.emb_quantize(tables[1], bits)                       # (code object load)
        torch.cuda.synchronize()
        q = []
        pack_ms[bits] = time_ms(lambda: q.extend(ops.emb_quantize(w, bits) for w in tables))
        packed[bits] = q
    offs = [torch.arange(B, device=dev, dtype=idt) * h for h in hot]
    idxs = [torch.randint(0, n, (B * h,), device=dev, generator=g).to(idt) for n, h in zip(rows, hot)]
    bags = ops.BagBatch(offs, idxs)
    out = torch.empty((B, T * D), dtype=torch.float32, device=dev)
    kernels = {
        "dlrm_emb_fwd (fp32)": lambda: ops.emb_fwd(tables, bags, out),
        "dlrm_emb_fwd_quant 8-bit": lambda: ops.emb_fwd_quant(packed[8], rows, D, 8, bags, out),
        "dlrm_emb_fwd_quant 4-bit": lambda: ops.emb_fwd_quant(packed[4], rows, D, 4, bags, out),
    }
    row_bytes = {"dlrm_emb_fwd (fp32)": 4 * D, "dlrm_emb_fwd_quant 8-bit": D + 8, "dlrm_emb_fwd_quant 4-bit": D // 2 + 4}
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
    out_bytes = B * T * D * 4
    idx_bytes = nnz * isz + B * T * isz
    lines.append("")
    lines.append("### %s: %d tables, D = %d, B = %d, %d lookups per sample, %s ids%s" %
                 (name, T, D, B, sum(hot), "int32" if isz == 4 else "int64", "" if args.scale == 1.0 else " — TABLES SCALED BY %g (rehearsal)" % args.scale))
    lines.append("")
    lines.append("| kernel | median ms | min | max | index MB | row MB | output MB | algorithmic GB/s | vs fp32 |")
    lines.append("|---|---|---|---|---|---|---|---|---|")
    base = statistics.median(times["dlrm_emb_fwd (fp32)"])
    for k in kernels:
        med = statistics.median(times[k])
        rb = nnz * row_bytes[k]
        total = idx_bytes + rb + out_bytes
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.1f | %.1f | %.0f | %.2fx |" %
                     (k, med, min(times[k]), max(times[k]), idx_bytes / 1e6, rb / 1e6, out_bytes / 1e6, total / med / 1e6, base / med))
    n_rows = sum(rows)
    for bits in (8, 4):
        moved = n_rows * (4 * D + row_bytes["dlrm_emb_fwd_quant %d-bit" % bits])
        lines.append("")
        lines.append("dlrm_emb_quantize_rows %d-bit, all %d tables (%.1f GB fp32 -> %.1f GB packed, one pass, timed once): %.1f ms, %.0f GB/s read + written" %
                     (bits, T, n_rows * 4 * D / 1e9, n_rows * row_bytes["dlrm_emb_fwd_quant %d-bit" % bits] / 1e9, pack_ms[bits], moved / pack_ms[bits] / 1e6))
    del tables, packed, kernels, bags
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["criteo_terabyte", "mlperf_v2_multihot", "both"])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_quant_emb.py measures on the GPU; none found")
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
