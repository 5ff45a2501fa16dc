#!/usr/bin/env python3
"""The fused QR lookup + interaction kernels (forward and backward) beside the two-kernel form they replace and beside the plain fp32 fused
kernels, same process, same GPU, same ids.

    python tools/bench_qr_interact.py [--repeats 20] [--warmup 3] [--max-rows 10000000] [--collisions 4] [--threshold 200]
                                      [--out profiles/qr_emb/fused_interact_rates.md]

Shapes: Criteo-Terabyte (bench.py WORKLOADS: 26 tables, D = 128, B = 65536, one lookup per bag, int64 ids; row counts capped at --max-rows
per table so that the plain fp32 tables and the QR tables are resident together).  Every table with more than --threshold rows is a QR
table of --collisions collisions (18 of the 26 at the defaults), the rest stay plain; both operations ("mult", "add") are measured.
  forward : dlrm_interact_fwd_gather_qr (fused);  dlrm_emb_fwd_qr — keeping the two pooled sums for the backward when the operation is
            "mult", as a training step does — + dlrm_interact_fwd over the buffer the lookup wrote (both launches inside one timed
            interval, and the lookup alone);  dlrm_interact_fwd_gather (plain fp32 tables of the capped full row counts, fused) for scale.
  backward: dlrm_interact_bwd_gather_qr (fused; for "mult" it includes its second launch);  dlrm_interact_bwd over (x, the pooled buffer)
            + dlrm_emb_qr_bwd_split (both inside one timed interval);  dlrm_interact_bwd_gather (plain fp32, fused) for scale.

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each variant once between two HIP events (the
variants alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported with min / max.  Before timing, the
fused results are compared with the two-kernel results bit for bit.  Algorithmic bytes: ids + offsets, table row bytes (a weight_q row per
lookup; weight_r is c rows and is counted once), x, R / dR, dx and the gradient buffer of the virtual table list; the two-kernel form adds
the [B, T*D] fp32 buffer (forward: written and read back; backward: its gradient written and read back) and, for "mult", the
[B, 2*Tq*D] sums (forward: written; backward: read).  No GPU: the tool fails."""
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


def run_op(op, name, rows, B, args, dev, lines, shared):
    from dlrm_amd import ops
    D, T, c = 128, len(rows), args.collisions
    F = T + 1
    coll = [c if n > args.threshold else 0 for n in rows]
    Tq = sum(1 for k in coll if k)
    Tv = T + Tq
    plain, Wq, Wr, bags, x, dR, ldr = shared
    Wd = ops.interact_out_width(F, D, 0)
    feat = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    feat[:, :D] = x
    E = feat[:, D:]
    saved = torch.empty((B, 2 * Tq * D), dtype=torch.float32, device=dev) if op == "mult" else None
    R = {k: torch.empty((B, ldr), dtype=torch.float32, device=dev) for k in ("fused", "two", "fp32")}
    dx = {k: torch.empty((B, D), dtype=torch.float32, device=dev) for k in ("fused", "two", "fp32")}
    gout = {k: torch.empty((B, Tv * D), dtype=torch.float32, device=dev) for k in ("fused", "two")}
    dE = {k: torch.empty((B, T * D), dtype=torch.float32, device=dev) for k in ("two", "fp32")}
    mode = ops.INTERACT_RELU_X          # what the model's backward passes (the bottom tower ends in a ReLU)

    def two_fwd():
        ops.emb_fwd_qr(Wq, Wr, rows, coll, op, bags, E, saved)
        ops.interact_fwd((feat,), D, 0, R["two"])

    def two_bwd():
        ops.interact_bwd((x, E), D, mode, dR, (dx["two"], dE["two"]))
        ops.emb_qr_bwd_split(coll, op, D, dE["two"], saved, gout["two"])
    kernels = {
        "forward: QR fused (dlrm_interact_fwd_gather_qr)": lambda: ops.interact_fwd_gather_qr(x, Wq, Wr, rows, coll, op, bags, D, 0, R["fused"]),
        "forward: QR two kernels (dlrm_emb_fwd_qr + dlrm_interact_fwd)": two_fwd,
        "forward: QR lookup alone (dlrm_emb_fwd_qr)": lambda: ops.emb_fwd_qr(Wq, Wr, rows, coll, op, bags, E, saved),
        "forward: plain fp32 fused (dlrm_interact_fwd_gather)": lambda: ops.interact_fwd_gather(x, plain, bags, D, 0, R["fp32"]),
        "backward: QR fused (dlrm_interact_bwd_gather_qr)":
            lambda: ops.interact_bwd_gather_qr(x, Wq, Wr, rows, coll, op, bags, D, mode, dR, dx["fused"], gout["fused"]),
        "backward: QR two-kernel form (dlrm_interact_bwd + dlrm_emb_qr_bwd_split)": two_bwd,
        "backward: plain fp32 fused (dlrm_interact_bwd_gather)": lambda: ops.interact_bwd_gather(x, plain, bags, D, mode, dR, dx["fp32"], dE["fp32"]),
    }
    # the results the timed kernels compute are the same bits
    for fn in kernels.values():
        fn()
    ops.check_index_errors(sync=True)
    if not same_bits(R["fused"], R["two"]) or not same_bits(dx["fused"], dx["two"]) or not same_bits(gout["fused"], gout["two"]):
        sys.exit("ERROR: %s, %s: the fused QR kernels and the two-kernel form differ" % (name, op))
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
    xb, rb, buf, gb = B * D * 4, B * ldr * 4, B * T * D * 4, B * Tv * D * 4
    sums = B * 2 * Tq * D * 4 if op == "mult" else 0
    rows_qr = B * T * 4 * D + Tq * c * D * 4           # one weight_q / plain row per lookup; weight_r once per table
    rows32 = B * T * 4 * D
    total = {
        "forward: QR fused (dlrm_interact_fwd_gather_qr)": sel + rows_qr + xb + rb,
        "forward: QR two kernels (dlrm_emb_fwd_qr + dlrm_interact_fwd)": sel + rows_qr + 2 * buf + sums + xb + rb,
        "forward: QR lookup alone (dlrm_emb_fwd_qr)": sel + rows_qr + buf + sums,
        "forward: plain fp32 fused (dlrm_interact_fwd_gather)": sel + rows32 + xb + rb,
        # "mult": the second launch reads the ids and the rows again, reads the q slots and writes both slots of every QR table
        "backward: QR fused (dlrm_interact_bwd_gather_qr)": sel + rows_qr + xb + rb + xb + gb
            + ((B * Tq * 8 + B * Tq * 4 * D + B * Tq * D * 4) if op == "mult" else 0),
        "backward: QR two-kernel form (dlrm_interact_bwd + dlrm_emb_qr_bwd_split)": buf + xb + rb + xb + 2 * buf + sums + gb,
        "backward: plain fp32 fused (dlrm_interact_bwd_gather)": sel + rows32 + xb + rb + xb + buf,
    }
    lines.append("")
    lines.append("### %s, operation \"%s\": %d tables (%d QR at c = %d, %.1f M categories, at most %d per table), D = 128, B = %d, one lookup "
                 "per bag, int64 ids" % (name, op, T, Tq, c, sum(rows) / 1e6, max(rows), B))
    lines.append("")
    lines.append("| kernel | median ms | min | max | algorithmic MB | GB/s |")
    lines.append("|---|---|---|---|---|---|")
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.0f |" % (k, med[k], min(ts), max(ts), total[k] / 1e6, total[k] / med[k] / 1e6))
    lines.append("")
    for what in ("forward", "backward"):
        f = med[[k for k in med if k.startswith(what) and "QR fused" in k][0]]
        t = med[[k for k in med if k.startswith(what) and "two" in k][0]]
        p = med[[k for k in med if k.startswith(what) and "fp32 fused" in k][0]]
        lines.append("%s, \"%s\": QR fused %.4f ms, two-kernel form %.4f ms (fused is %.2fx %s), plain fp32 fused %.4f ms (QR fused is %.2fx %s)" %
                     (what, op, f, t, t / f if f <= t else f / t, "faster" if f < t else "SLOWER", p, p / f if f <= p else f / p,
                      "faster" if f < p else "SLOWER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=10_000_000, help="cap of every table's row count (plain fp32 + QR tables stay resident)")
    ap.add_argument("--collisions", type=int, default=4)
    ap.add_argument("--threshold", type=int, default=200, help="tables with more rows are QR tables (the reference's --qr-threshold)")
    ap.add_argument("--batch", type=int, default=0, help="batch size (default: the workload's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_qr_interact.py measures on the GPU; none found")
    import bench
    from dlrm_amd import ops
    dev = torch.device("cuda:0")
    name = "criteo_terabyte"
    rows = [min(n, args.max_rows) for n in bench.WORKLOADS[name]["rows"]]
    B = args.batch or bench.WORKLOADS[name]["batch"]
    D, T, c = 128, len(rows), args.collisions
    g = torch.Generator(device=dev).manual_seed(7)
    coll = [c if n > args.threshold else 0 for n in rows]
    plain = [torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-float(n) ** -0.5, float(n) ** -0.5, generator=g) for n in rows]
    Wq = [torch.empty((ops.qr_rows_q(n, c), D), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=g) if coll[t] else plain[t]
          for t, n in enumerate(rows)]
    Wr = [torch.empty((c, D), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=g) if coll[t] else None for t in range(T)]
    offs = [ops.mark_one_lookup_per_bag(torch.arange(B, device=dev)) for _ in rows]
    idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    x = torch.randn((B, D), device=dev, generator=g)
    Wd = ops.interact_out_width(T + 1, D, 0)
    ldr = (Wd + 3) & ~3
    dR = torch.zeros((B, ldr), dtype=torch.float32, device=dev)
    dR[:, :Wd] = torch.randn((B, Wd), device=dev, generator=g)
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median; all kernels in one process, alternating inside every round" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup)]
    for op in ("mult", "add"):
        run_op(op, name, rows, B, args, dev, lines, (plain, Wq, Wr, bags, x, dR, ldr))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
