#!/usr/bin/env python3
"""Forward time of the MLP towers with fp32, bf16, int8 and fp16-rounded weights, same process, same GPU, same inputs.

    python tools/bench_quant_mlp.py [--shape criteo_terabyte|criteo_kaggle|both] [--repeats 30] [--inner 20] [--warmup 5] [--out FILE.md]

Towers (bench.py WORKLOADS): Criteo-Terabyte 13-512-256-128 and 479-1024-1024-512-256-1 at B = 65536, Criteo-Kaggle 13-512-256-64-16 and
the top tower its interaction feeds, at B = 2048.  Variants: FusedMLP with arith "f32" and "bf16" (forward only, no autograd), the
same tower after quantize(8) (per layer: range pass, quantise pass, int8 GEMM) and after quantize(16) (fp16-rounded weights on the fp32 path).

Protocol (docs/MEASUREMENT.md): warm-up forwards, then `repeats` rounds; every round times each variant once — `inner` back-to-back
forwards between two HIP events, divided by `inner`, so that a sample is milliseconds of queued work and not one launch's latency (the
variants alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported, with min / max.  The per-layer split of
the int8 tower times the three launches of each layer the same way, on the layer's real input.  A measurement path that finds no GPU fails."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def time_ms(fn, inner: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def med(ts):
    return statistics.median(ts), min(ts), max(ts)


def run_tower(title, ln, sigmoid_layer, x, args, lines):
    import dlrm_amd
    from dlrm_amd import ops
    dev = x.device
    B = x.size(0)

    def make(arith=None, bits=32):
        np.random.seed(11)
        t = dlrm_amd.DLRM_Net().create_mlp(np.asarray(ln), sigmoid_layer).to(dev)
        if arith:
            t.arith = arith
        t.quantize(bits)
        return t

    towers = {"f32": make("f32"), "bf16": make("bf16"), "int8 (quantize 8)": make(bits=8), "fp16 weights (quantize 16)": make(bits=16)}
    with torch.no_grad():
        for _ in range(args.warmup):
            for t in towers.values():
                t(x)
        torch.cuda.synchronize()
        times = {k: [] for k in towers}
        for _ in range(args.repeats):
            for k, t in towers.items():
                times[k].append(time_ms(lambda: t(x), args.inner))
    flop = 2.0 * B * sum(int(ln[i]) * int(ln[i + 1]) for i in range(len(ln) - 1))
    lines += ["", "### %s: %s, B = %d (%.3f TFLOP per forward)" % (title, "-".join(str(int(v)) for v in ln), B, flop / 1e12), "",
              "| towers' weights | median ms | min | max | TFLOP/s | vs f32 | vs bf16 |", "|---|---|---|---|---|---|---|"]
    base, b16 = statistics.median(times["f32"]), statistics.median(times["bf16"])
    for k in towers:
        m, lo, hi = med(times[k])
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.2fx | %.2fx |" % (k, m, lo, hi, flop / m / 1e9, base / m, b16 / m))
    # the int8 tower layer by layer, each launch on the layer's real input
    q = towers["int8 (quantize 8)"]
    params, acts = q._layers()
    lines += ["", "| int8 layer | range ms | quantise ms | GEMM ms | GEMM TOP/s |", "|---|---|---|---|---|"]
    cur = x
    with torch.no_grad():
        for i, W in enumerate(q._q8):
            bufs = ops.q8_quantize_act(cur, W.K)
            out = torch.empty((B, W.N), dtype=torch.float32, device=dev)
            bias = params[2 * i + 1].detach()
            steps = {"range": lambda: ops.q8_quantize_act(cur, W.K, ops.Q8_RANGE, bufs),
                     "quantise": lambda: ops.q8_quantize_act(cur, W.K, ops.Q8_QUANTIZE, bufs),
                     "gemm": lambda: ops.gemm_q8(bufs[0], bufs[1], W, bias, acts[i], out)}
            for _ in range(args.warmup):
                for fn in steps.values():
                    fn()
            ts = {k: [] for k in steps}
            for _ in range(args.repeats):
                for k, fn in steps.items():
                    ts[k].append(time_ms(fn, args.inner))
            g = statistics.median(ts["gemm"])
            lines.append("| %d -> %d | %.4f | %.4f | %.4f | %.1f |" % (W.K, W.N, statistics.median(ts["range"]), statistics.median(ts["quantise"]), g,
                                                                   2.0 * B * W.K * W.N / g / 1e9))
            cur = out
    del towers
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["criteo_terabyte", "criteo_kaggle", "both"])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="forwards (or launches) per timed sample")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_quant_mlp.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats of %d back-to-back runs each after %d warm-up rounds, HIP events, median of the per-run time" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.inner, args.warmup)]
    g = torch.Generator(device=dev).manual_seed(3)
    for name in (["criteo_terabyte", "criteo_kaggle"] if args.shape == "both" else [args.shape]):
        wl = bench.WORKLOADS[name]
        B, D, F = wl["batch"], wl["D"], len(wl["rows"]) + 1
        k_top = D + F * (F - 1) // 2
        xb = torch.rand((B, wl["bot"][0]), device=dev, generator=g)
        run_tower(name + " bottom tower", wl["bot"], -1, xb, args, lines)
        # the top tower's input as the interaction emits it: [B, round4(width)], zero padded, signed values
        xt = torch.zeros((B, (k_top + 3) & ~3), device=dev)
        xt[:, :k_top] = torch.randn((B, k_top), device=dev, generator=g)
        top = [k_top] + list(wl["top"])
        run_tower(name + " top tower", top, len(top) - 2, xt, args, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
