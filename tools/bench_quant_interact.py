#!/usr/bin/env python3
"""The fused quantised lookup + interaction forward beside the two-kernel form it replaces, same process, same GPU, same inputs.

    python tools/bench_quant_interact.py [--repeats 30] [--warmup 5] [--max-rows 10000000] [--out FILE.md]

Shapes: Criteo-Terabyte (bench.py WORKLOADS: 26 tables, D = 128, B = 65536, one lookup per bag, int64 ids; row counts capped at --max-rows
per table so that the fp32 tables and both packed forms are resident together) and a Kaggle-like small batch (Criteo-Kaggle row counts,
the same cap, D = 128, B = 2048).  Per bits in {8, 4}: dlrm_interact_fwd_gather_quant (fused), dlrm_emb_fwd_quant, dlrm_interact_fwd over the
buffer the lookup wrote, and the sum of those two; also dlrm_interact_fwd_gather (fp32, fused) on the unquantised tables of the same shape.

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each kernel once between two HIP events (the
kernels alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported with min / max.  "two kernels" is the
per-round sum of the lookup and the interaction.  Before timing, the fused result is compared with the two-kernel result bit for bit.
Algorithmic bytes: ids + offsets, packed (or fp32) row bytes, x, and R; the two-kernel form adds the [B, T*D] fp32 buffer written and read
back.  A measurement path that finds no GPU fails."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def time_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_shape(name, rows, B, args, dev, lines, verdict):
    from dlrm_amd import ops
    D, T = 128, len(rows)
    F = T + 1
    g = torch.Generator(device=dev).manual_seed(7)
    tables = [torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-float(n) ** -0.5, float(n) ** -0.5, generator=g) for n in rows]
    packed = {bits: [ops.emb_quantize(w, bits) for w in tables] for bits in (8, 4)}
    offs = [ops.mark_one_lookup_per_bag(torch.arange(B, device=dev)) for _ in rows]
    idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    x = torch.randn((B, D), device=dev, generator=g)
    ldr = (ops.interact_out_width(F, D, 0) + 3) & ~3
    feat = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    feat[:, :D] = x
    R = {k: torch.empty((B, ldr), dtype=torch.float32, device=dev) for k in ("fused", "two", "fp32")}
    kernels = {"fp32 fused (dlrm_interact_fwd_gather)": lambda: ops.interact_fwd_gather(x, tables, bags, D, 0, R["fp32"])}
    for bits in (8, 4):
        kernels["%d-bit fused (dlrm_interact_fwd_gather_quant)" % bits] = \
            lambda bits=bits: ops.interact_fwd_gather_quant(x, packed[bits], rows, D, bits, bags, 0, R["fused"])
        kernels["%d-bit lookup (dlrm_emb_fwd_quant)" % bits] = lambda bits=bits: ops.emb_fwd_quant(packed[bits], rows, D, bits, bags, feat[:, D:])
        kernels["%d-bit interaction (dlrm_interact_fwd)" % bits] = lambda: ops.interact_fwd((feat,), D, 0, R["two"])
    # the results the timed kernels compute are the same bits
    for bits in (8, 4):
        kernels["%d-bit fused (dlrm_interact_fwd_gather_quant)" % bits]()
        kernels["%d-bit lookup (dlrm_emb_fwd_quant)" % bits]()
        kernels["%d-bit interaction (dlrm_interact_fwd)" % bits]()
        ops.check_index_errors(sync=True)
        if not torch.equal(R["fused"].view(torch.int32), R["two"].view(torch.int32)):
            sys.exit("ERROR: %s, %d bits: the fused kernel and the two-kernel form differ" % (name, bits))
    for _ in range(args.warmup):
        for fn in kernels.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in kernels}
    for _ in range(args.repeats):
        for k, fn in kernels.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    for bits in (8, 4):
        a, b = times["%d-bit lookup (dlrm_emb_fwd_quant)" % bits], times["%d-bit interaction (dlrm_interact_fwd)" % bits]
        times["%d-bit two kernels (lookup + interaction)" % bits] = [u + v for u, v in zip(a, b)]
    sel = 2 * B * T * 8
    xb, rb, buf = B * D * 4, B * ldr * 4, B * T * D * 4
    row = {"fp32": 4 * D, "8-bit": D + 8, "4-bit": D // 2 + 4}
    lines.append("")
    lines.append("### %s: %d tables (%.1f M rows, at most %d per table), D = 128, B = %d, one lookup per bag, int64 ids" %
                 (name, T, sum(rows) / 1e6, max(rows), B))
    lines.append("")
    lines.append("| kernel | median ms | min | max | algorithmic MB | GB/s |")
    lines.append("|---|---|---|---|---|---|")
    med = {}
    for k, ts in times.items():
        kind = k.split(" ")[0]
        if "lookup (" in k:
            total = sel + B * T * row[kind] + buf
        elif "interaction (" in k:
            total = buf + xb + rb
        elif "two kernels" in k:
            total = sel + B * T * row[kind] + 2 * buf + xb + rb
        else:
            total = sel + B * T * row[kind] + xb + rb
        med[k] = statistics.median(ts)
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.0f |" % (k, med[k], min(ts), max(ts), total / 1e6, total / med[k] / 1e6))
    lines.append("")
    for bits in (8, 4):
        f, t = med["%d-bit fused (dlrm_interact_fwd_gather_quant)" % bits], med["%d-bit two kernels (lookup + interaction)" % bits]
        lines.append("%d bits: fused %.4f ms, two kernels %.4f ms: fused is %.2fx %s; fp32 fused %.4f ms" %
                     (bits, f, t, t / f if f <= t else f / t, "faster" if f < t else "SLOWER", med["fp32 fused (dlrm_interact_fwd_gather)"]))
        verdict.append(f < t)
    del tables, packed, kernels, bags, feat, R
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=10_000_000, help="cap of every table's row count (fp32 + both packed forms stay resident)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_quant_interact.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median; all kernels of a shape in one process, alternating" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup)]
    tb, small = [], []
    run_shape("criteo_terabyte", [min(n, args.max_rows) for n in bench.WORKLOADS["criteo_terabyte"]["rows"]],
              bench.WORKLOADS["criteo_terabyte"]["batch"], args, dev, lines, tb)
    run_shape("kaggle_like_b2048", [min(n, args.max_rows) for n in bench.WORKLOADS["criteo_kaggle"]["rows"]],
              bench.WORKLOADS["criteo_kaggle"]["batch"], args, dev, lines, small)
    lines.append("")
    lines.append("Default of DLRM_Net.fuse_quant_interact by the rule (fused faster than the two kernels at Criteo-Terabyte shapes at BOTH widths): %s"
                 % ("True" if all(tb) else "False"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
