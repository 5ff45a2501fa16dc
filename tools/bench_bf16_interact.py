#!/usr/bin/env python3
"""The fused bf16 lookup + interaction kernels (forward and backward) beside the two-kernel form they replace and beside the fp32 fused
kernels, same process, same GPU, same inputs.

    python tools/bench_bf16_interact.py [--repeats 20] [--warmup 3] [--max-rows 10000000] [--out profiles/bf16_emb/fused_interact_rates.md]

Shapes: Criteo-Terabyte (bench.py WORKLOADS: 26 tables, D = 128, B = 65536, one lookup per bag, int64 ids; row counts capped at --max-rows
per table so that the fp32 and the bf16 tables are resident together).
  forward : dlrm_interact_fwd_gather_bf16 (fused);  dlrm_emb_fwd_bf16 + dlrm_interact_fwd over the buffer the lookup wrote (both launches
            inside one timed interval, and the lookup alone);  dlrm_interact_fwd_gather (fp32, fused) on the upcast tables.
  backward: dlrm_interact_bwd_gather_bf16 (fused);  dlrm_interact_bwd over (x, the pooled buffer) — the backward of the two-kernel form;
            dlrm_interact_bwd_gather (fp32, fused) on the upcast tables.

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each variant once between two HIP events (the
variants alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported with min / max.  Before timing, the
fused results are compared with the two-kernel results bit for bit.  Algorithmic bytes: ids + offsets, table row bytes, x, R / dR, dx and
dE; the two-kernel form adds the [B, T*D] fp32 buffer (forward: written and read back; backward: read).  No GPU: the tool fails."""
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


def same_bits(a, b) -> bool:
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_shape(name, rows, B, args, dev, lines):
    from dlrm_amd import ops
    D, T = 128, len(rows)
    F = T + 1
    g = torch.Generator(device=dev).manual_seed(7)
    bf16 = []
    for n in rows:
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-float(n) ** -0.5, float(n) ** -0.5, generator=g)
        bf16.append(w.to(torch.bfloat16))
        del w
    fp32 = [w.float() for w in bf16]
    offs = [ops.mark_one_lookup_per_bag(torch.arange(B, device=dev)) for _ in rows]
    idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    x = torch.randn((B, D), device=dev, generator=g)
    Wd = ops.interact_out_width(F, D, 0)
    ldr = (Wd + 3) & ~3
    feat = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    feat[:, :D] = x
    E = feat[:, D:]
    dR = torch.zeros((B, ldr), dtype=torch.float32, device=dev)
    dR[:, :Wd] = torch.randn((B, Wd), device=dev, generator=g)
    R = {k: torch.empty((B, ldr), dtype=torch.float32, device=dev) for k in ("fused", "two", "fp32")}
    G = {k: (torch.empty((B, D), dtype=torch.float32, device=dev), torch.empty((B, T * D), dtype=torch.float32, device=dev))
         for k in ("fused", "two", "fp32")}
    mode = ops.INTERACT_RELU_X          # what the model's backward passes (the bottom tower ends in a ReLU)

    def two_fwd():
        ops.emb_fwd_bf16(bf16, bags, E)
        ops.interact_fwd((feat,), D, 0, R["two"])
    kernels = {
        "forward: bf16 fused (dlrm_interact_fwd_gather_bf16)": lambda: ops.interact_fwd_gather(x, bf16, bags, D, 0, R["fused"]),
        "forward: bf16 two kernels (dlrm_emb_fwd_bf16 + dlrm_interact_fwd)": two_fwd,
        "forward: bf16 lookup alone (dlrm_emb_fwd_bf16)": lambda: ops.emb_fwd_bf16(bf16, bags, E),
        "forward: fp32 fused (dlrm_interact_fwd_gather)": lambda: ops.interact_fwd_gather(x, fp32, bags, D, 0, R["fp32"]),
        "backward: bf16 fused (dlrm_interact_bwd_gather_bf16)": lambda: ops.interact_bwd_gather(x, bf16, bags, D, mode, dR, *G["fused"]),
        "backward: bf16 two-kernel form (dlrm_interact_bwd)": lambda: ops.interact_bwd((x, E), D, mode, dR, G["two"]),
        "backward: fp32 fused (dlrm_interact_bwd_gather)": lambda: ops.interact_bwd_gather(x, fp32, bags, D, mode, dR, *G["fp32"]),
    }
    # the results the timed kernels compute are the same bits
    for fn in kernels.values():
        fn()
    ops.check_index_errors(sync=True)
    for k in ("two", "fp32"):
        if not same_bits(R["fused"], R[k]) or not same_bits(G["fused"][0], G[k][0]) or not same_bits(G["fused"][1], G[k][1]):
            sys.exit("ERROR: %s: the fused bf16 kernels and the %s form differ" % (name, k))
    for _ in range(args.warmup):
        for fn in kernels.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in kernels}
    for _ in range(args.repeats):
        for k, fn in kernels.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    sel = 2 * B * T * 8
    xb, rb, buf = B * D * 4, B * ldr * 4, B * T * D * 4
    grads = xb + buf                          # dx + dE
    rows16, rows32 = B * T * 2 * D, B * T * 4 * D
    total = {
        "forward: bf16 fused (dlrm_interact_fwd_gather_bf16)": sel + rows16 + xb + rb,
        "forward: bf16 two kernels (dlrm_emb_fwd_bf16 + dlrm_interact_fwd)": sel + rows16 + 2 * buf + xb + rb,
        "forward: bf16 lookup alone (dlrm_emb_fwd_bf16)": sel + rows16 + buf,
        "forward: fp32 fused (dlrm_interact_fwd_gather)": sel + rows32 + xb + rb,
        "backward: bf16 fused (dlrm_interact_bwd_gather_bf16)": sel + rows16 + xb + rb + grads,
        "backward: bf16 two-kernel form (dlrm_interact_bwd)": buf + xb + rb + grads,
        "backward: fp32 fused (dlrm_interact_bwd_gather)": sel + rows32 + xb + rb + grads,
    }
    lines.append("")
    lines.append("### %s: %d tables (%.1f M rows, at most %d per table), D = 128, B = %d, one lookup per bag, int64 ids" %
                 (name, T, sum(rows) / 1e6, max(rows), B))
    lines.append("")
    lines.append("| kernel | median ms | min | max | algorithmic MB | GB/s |")
    lines.append("|---|---|---|---|---|---|")
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.0f |" % (k, med[k], min(ts), max(ts), total[k] / 1e6, total[k] / med[k] / 1e6))
    lines.append("")
    for what in ("forward", "backward"):
        f = med[[k for k in med if k.startswith(what) and "bf16 fused" in k][0]]
        t = med[[k for k in med if k.startswith(what) and "two" in k][0]]
        p = med[[k for k in med if k.startswith(what) and "fp32 fused" in k][0]]
        lines.append("%s: bf16 fused %.4f ms, two-kernel form %.4f ms (fused is %.2fx %s), fp32 fused %.4f ms (bf16 fused is %.2fx %s)" %
                     (what, f, t, t / f if f <= t else f / t, "faster" if f < t else "SLOWER", p, p / f if f <= p else f / p,
                      "faster" if f < p else "SLOWER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=10_000_000, help="cap of every table's row count (fp32 + bf16 tables stay resident)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_bf16_interact.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median; all kernels in one process, alternating inside every round" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup)]
    run_shape("criteo_terabyte", [min(n, args.max_rows) for n in bench.WORKLOADS["criteo_terabyte"]["rows"]],
              bench.WORKLOADS["criteo_terabyte"]["batch"], args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
