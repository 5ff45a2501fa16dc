#!/usr/bin/env python3
"""Times the sorted-walk embedding updates at lane shapes the other benchmarks never launch: launch groups with 64-bit sort keys (32 tables, one
of them with more than 2^27 rows) and the one-column-per-lane kernels of unaligned widths.  One markdown table, medians of HIP-event times in ms.
    python tools/bench_walk_shapes.py [--repeats 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BIG = (1 << 27) + 1          # rows of the table that makes row bits + table bits exceed 32

# name, update, D, rows of table 0 (the other 31 tables: 100000 rows), kernel the groups pass launches
CASES = [
    ("fp32 row-wise, D = 6, 64-bit keys", "rowwise", 6, BIG, "adagrad_groups_kernel<1, 8, 1, u64, 2, false>"),
    ("fp32 exact, D = 4, 64-bit keys", "exact", 4, BIG, "adagrad_groups_kernel<4, 4, 1, u64, 2, true>"),
    ("bf16 row-wise, D = 4, 64-bit keys", "bf16", 4, BIG, "bf16_groups_kernel<4, 4, 1, u64, true>"),
    ("bf16 row-wise, D = 256, 64-bit keys", "bf16", 256, BIG, "bf16_groups_kernel<4, 64, 1, u64, true>"),
    ("bf16 row-wise, D = 30, 32-bit keys", "bf16", 30, 100000, "bf16_groups_kernel<1, 32, 1, u32, true>"),
    ("fp32 exact, D = 14, 32-bit keys", "exact", 14, 100000, "adagrad_groups_kernel<1, 16, 1, u32, 2, true>"),
    ("fp32 row-wise, D = 128, 32-bit keys (the benchmarks' shape)", "rowwise", 128, 100000, "adagrad_groups_kernel<4, 32, 1, u32, 2, false>"),
]


def time_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run_case(kind, D, rows0, B, args, dev):
    from dlrm_amd import ops
    T = 32
    rows = [rows0] + [100000] * (T - 1)
    g = torch.Generator(device=dev).manual_seed(11)
    wdt = torch.bfloat16 if kind == "bf16" else torch.float32
    W = [torch.zeros((n, D), dtype=wdt, device=dev) for n in rows]
    state = [torch.zeros((n, D) if kind == "exact" else (n,), dtype=torch.float32, device=dev) for n in rows]
    offs = [torch.arange(B, device=dev, dtype=torch.int64) for _ in rows]
    idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    dout = torch.empty((B, T * D), dtype=torch.float32, device=dev).uniform_(-1e-3, 1e-3, generator=g)
    if kind == "rowwise":
        fn = lambda: ops.emb_bwd_rowwise_adagrad(W, state, bags, dout, 1e-3, 1e-8)
    elif kind == "exact":
        fn = lambda: ops.emb_bwd_adagrad(W, state, bags, dout, 1e-3, 1e-8)
    else:
        fn = lambda: ops.emb_bwd_rowwise_adagrad_bf16(W, state, bags, dout, 1e-3, 1e-8, "nearest", 0)
    for _ in range(args.warmup):
        fn()
    ops.check_index_errors(sync=True)
    t = [time_ms(fn) for _ in range(args.repeats)]
    ops.check_index_errors(sync=True)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_walk_shapes.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup), "",
             "### walk shapes: 32 tables, B = %d, one lookup per bag, int64 ids" % args.batch, "",
             "| update (sort + both passes) | groups kernel | median ms | min | max |", "|---|---|---|---|---|"]
    for name, kind, D, rows0, kernel in CASES:
        med, lo, hi = run_case(kind, D, rows0, args.batch, args, dev)
        torch.cuda.empty_cache()
        lines.append("| %s | `%s` | %.4f | %.4f | %.4f |" % (name, kernel, med, lo, hi))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
