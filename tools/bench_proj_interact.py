#!/usr/bin/env python3
"""The projected interaction kernels of DLRM_Projection (dlrm_proj_interact_fwd / _bwd, csrc/interact_proj.hip) beside the stock composition
they replace — torch.bmm on reshaped views + torch.cat, and autograd's backward of it — same process, same GPU, same inputs.

    python tools/bench_proj_interact.py [--repeats 30] [--warmup 3] [--out profiles/proj_interact/rates.md]

Shapes: (I1, I2, D) = (16, 16, 128) and (32, 32, 64) — the trainer's default branch sizes 2048 at the two embedding widths — each at
B = 2048 and B = 65536.

Protocol (docs/MEASUREMENT.md): every variant runs over a ring of operand sets whose total size exceeds twice the 256 MiB last-level cache (at
least 2 sets), so no call finds its operands cached by the call before it.  One timed interval is one pass over the ring between two HIP
events; the per-call time is the interval over the ring length.  Warm-up rounds, then `repeats` rounds in which the variants alternate (drift
hits all alike); the MEDIAN over the rounds is reported with min / max.  Before timing, the library's results are compared with the stock
composition's (fp32 round-off bounds of the kernel tests).  The box's copy rate is measured in the same run by dlrm_calib_hbm_copy
(2 x bytes / time over 1 GiB) in front of and behind the timed rounds; "of copy" is a kernel's algorithmic bytes per second over the smaller of
the two.  Algorithmic bytes per sample — forward: x, P1, P2 read, R written; backward: P1, P2, dR read, dx, dP1, dP2 written.  The stock
composition's own traffic is larger (Z is written by bmm and read back by cat; autograd's backward materialises transposes): its GB/s column
uses the SAME algorithmic bytes, so the two columns compare times, not traffic.  No GPU: the tool fails."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

SHAPES = ((16, 16, 128), (32, 32, 64))
BATCHES = (2048, 65536)
RING_BYTES = 2 * 256 * 2 ** 20


def r4(n):
    return (n + 3) & ~3


def window_ms(fn, n) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(n):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def copy_rate_gbs(dev) -> float:
    from dlrm_amd import _lib
    lib = _lib.load()
    n = 2 ** 30
    a, b = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def one(_):
        _lib.check(lib.dlrm_calib_hbm_copy(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, st), "dlrm_calib_hbm_copy")
    window_ms(one, 3)
    ms = statistics.median(window_ms(one, 4) for _ in range(5))
    return 2 * n / ms / 1e6


def fwd_bytes(I1, I2, D):
    return 4 * (D + I1 * D + D * I2 + r4(D + I1 * I2))


def bwd_bytes(I1, I2, D):
    return 4 * (I1 * D + D * I2 + r4(D + I1 * I2) + D + I1 * D + D * I2)


def run_shape(I1, I2, D, B, args, dev, g, lines):
    from dlrm_amd import ops
    W, ldr = D + I1 * I2, r4(D + I1 * I2)
    per_set = B * max(fwd_bytes(I1, I2, D), bwd_bytes(I1, I2, D))
    n = max(2, -(-RING_BYTES // per_set))
    sets = []
    for _ in range(n):
        s = {"x": torch.randn((B, D), device=dev, generator=g), "P1": torch.randn((B, I1 * D), device=dev, generator=g),
             "P2": torch.randn((B, D * I2), device=dev, generator=g), "dR": torch.randn((B, ldr), device=dev, generator=g),
             "R": torch.empty((B, ldr), device=dev), "dx": torch.empty((B, D), device=dev), "dP1": torch.empty((B, I1 * D), device=dev),
             "dP2": torch.empty((B, D * I2), device=dev)}
        s["dR"][:, W:] = 0
        sets.append(s)

    def stock_fwd_of(s, leaves=False):
        x, P1, P2 = ((s[k].detach().requires_grad_(True) for k in ("x", "P1", "P2")) if leaves else (s["x"], s["P1"], s["P2"]))
        R = torch.cat([x, torch.bmm(P1.view(B, I1, D), P2.view(B, D, I2)).view(B, I1 * I2)], dim=1)
        return R, (x, P1, P2)
    graphs = [stock_fwd_of(s, leaves=True) for s in sets]          # autograd graphs of the stock forward, built outside the timed intervals

    def lib_fwd(k):
        s = sets[k % n]
        ops.proj_interact_fwd(s["x"], s["P1"], s["P2"], D, s["R"])

    def lib_bwd(k):
        s = sets[k % n]
        ops.proj_interact_bwd(s["P1"], s["P2"], D, s["dR"], s["dx"], s["dP1"], s["dP2"])

    def stock_fwd(k):
        stock_fwd_of(sets[k % n])

    def stock_bwd(k):
        R, leaves = graphs[k % n]
        return torch.autograd.grad(R, leaves, sets[k % n]["dR"][:, :W], retain_graph=True)
    # same results (fp32 round-off of a D-term dot of N(0, 1) data; the kernel tests hold the tight bounds against fp64)
    lib_fwd(0); lib_bwd(0)
    Rs, gs = stock_fwd_of(sets[0])[0], stock_bwd(0)
    s0 = sets[0]
    ok = torch.equal(s0["R"][:, :D], s0["x"]) and torch.allclose(s0["R"][:, :W], Rs, rtol=1e-4, atol=1e-4) and torch.equal(s0["dx"], gs[0]) \
        and torch.allclose(s0["dP1"], gs[1], rtol=1e-4, atol=1e-4) and torch.allclose(s0["dP2"], gs[2], rtol=1e-4, atol=1e-4)
    if not ok:
        sys.exit("ERROR: (%d, %d, %d) B = %d: the library's kernels and the stock composition differ" % (I1, I2, D, B))
    variants = {"forward: dlrm_proj_interact_fwd": (lib_fwd, fwd_bytes(I1, I2, D)), "forward: torch.bmm + torch.cat": (stock_fwd, fwd_bytes(I1, I2, D)),
                "backward: dlrm_proj_interact_bwd": (lib_bwd, bwd_bytes(I1, I2, D)),
                "backward: autograd of bmm + cat": (stock_bwd, bwd_bytes(I1, I2, D))}
    for _ in range(args.warmup):
        for fn, _b in variants.values():
            window_ms(fn, n)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (fn, _b) in variants.items():
            times[k].append(window_ms(fn, n))
    lines.append("")
    lines.append("### I1 = %d, I2 = %d, D = %d, B = %d (%d operand sets in the ring, %.0f MB each)" % (I1, I2, D, B, n, per_set / 1e6))
    lines.append("")
    lines.append("| kernel | median ms | min | max | algorithmic MB | GB/s | of copy |")
    lines.append("|---|---|---|---|---|---|---|")
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        mb = B * variants[k][1] / 1e6
        lines.append((k, med[k], min(ts), max(ts), mb))           # (formatted in main, once the copy rate behind the rounds is known)
    lines.append("")
    names = list(variants)
    for what, a, b in (("forward", names[0], names[1]), ("backward", names[2], names[3])):
        f, t = med[a], med[b]
        lines.append("%s: library %.4f ms, stock composition %.4f ms (the library is %.2fx %s)" %
                     (what, f, t, t / f if f <= t else f / t, "faster" if f < t else "SLOWER"))
    del sets, graphs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_proj_interact.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    before = copy_rate_gbs(dev)
    body = []
    for I1, I2, D in SHAPES:
        for B in BATCHES:
            run_shape(I1, I2, D, B, args, dev, g, body)
    after = copy_rate_gbs(dev)
    rate = min(before, after)
    body = [ln if isinstance(ln, str) else "| %s | %.4f | %.4f | %.4f | %.1f | %.0f | %.0f %% |" % (ln + (ln[4] / ln[1], 100 * ln[4] / ln[1] / rate))
            for ln in body]
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events around one pass over the operand ring, median; all variants in one "
             "process, alternating inside every round" % (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup),
             "", "copy rate of this box in this run (dlrm_calib_hbm_copy, 2 x 1 GiB / time): %.0f GB/s before, %.0f GB/s after the timed rounds; "
             "\"of copy\" is against %.0f GB/s" % (before, after, rate)] + body
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
