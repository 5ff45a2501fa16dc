#!/usr/bin/env python3
"""Lookup and update rates of quotient-remainder (QR) embedding tables beside plain fp32 tables, same process, same GPU, same ids.

    python tools/bench_qr_emb.py [--repeats 30] [--warmup 5] [--cap 8000000] [--collisions 4] [--threshold 200] [--hot 4] [--out FILE.md]

Shape: the 26 Criteo-Terabyte tables of bench.py (rows capped at --cap so that the fp32 tables, the QR tables and the buffers fit side by
side), D = 128, B = 65536, int64 ids; once with one lookup per bag and once with --hot lookups per bag.  Timed:
  (a) dlrm_emb_fwd on the fp32 tables of the (capped) full row count — the plain lookup, for scale;
  (b) the QR lookup composed from what existed before dlrm_emb_fwd_qr: dlrm_emb_fwd over the q tables (+ the plain tables), dlrm_emb_fwd over
      the r tables, one elementwise multiply.  The q / r id arrays are derived OUTSIDE the timed region (in (b)'s favour);
  (c) dlrm_emb_fwd_qr, writing the two pooled sums for the backward pass as in training;
  (d) the update: dlrm_emb_qr_bwd_split + dlrm_emb_qr_split_indices + dlrm_emb_bwd_sgd(SORTED) over the virtual tables, beside
      dlrm_emb_bwd_sgd(SORTED) over the plain tables (step size 0: the tables keep their values, the work is the same).
Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each candidate once between two HIP events (the
candidates alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported with min / max.  A measurement path
that finds no GPU fails."""
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


def table_bytes(rows_full, D, c, threshold):
    fp32 = sum(n * D * 4 for n in rows_full)
    qr = sum(((-(-n // c)) + c) * D * 4 if n > threshold else n * D * 4 for n in rows_full)
    return fp32, qr


def run(hot, rows, D, B, args, dev, lines):
    from dlrm_amd import ops
    c = args.collisions
    T = len(rows)
    coll = [c if n > args.threshold else 0 for n in rows]
    qr_t = [t for t in range(T) if coll[t]]
    g = torch.Generator(device=dev).manual_seed(7)
    plain = [torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-0.1, 0.1, generator=g) for n in rows]
    Wq = [torch.empty((ops.qr_rows_q(n, c), D), dtype=torch.float32, device=dev).uniform_(0.1, 1.0, generator=g) if coll[t] else plain[t]
          for t, n in enumerate(rows)]
    Wr = [torch.empty((c, D), dtype=torch.float32, device=dev).uniform_(0.1, 1.0, generator=g) if coll[t] else None for t in range(T)]
    offs = [torch.arange(B, device=dev, dtype=torch.int64) * hot for _ in rows]
    idxs = [torch.randint(0, n, (B * hot,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    out = torch.empty((B, T * D), dtype=torch.float32, device=dev)
    saved = torch.empty((B, 2 * len(qr_t) * D), dtype=torch.float32, device=dev)
    dout = torch.empty((B, T * D), dtype=torch.float32, device=dev).normal_(generator=g)
    # (b): QR tables first, so that the combine is one strided elementwise kernel
    order = qr_t + [t for t in range(T) if not coll[t]]
    qs, rs = ops.emb_qr_split_indices(rows, coll, bags)
    bags_q = ops.BagBatch([offs[t] for t in order], [qs[t] if coll[t] else idxs[t] for t in order])
    bags_r = ops.BagBatch([offs[t] for t in qr_t], [rs[t] for t in qr_t])
    Wq_b, Wr_b = [Wq[t] for t in order], [Wr[t] for t in qr_t]
    tmp = torch.empty((B, len(qr_t) * D), dtype=torch.float32, device=dev)

    def composed():
        ops.emb_fwd(Wq_b, bags_q, out)
        ops.emb_fwd(Wr_b, bags_r, tmp)
        out[:, :len(qr_t) * D].mul_(tmp)

    vw = []
    for t in range(T):
        vw += [Wq[t], Wr[t]] if coll[t] else [Wq[t]]

    def qr_update():
        gout = ops.emb_qr_bwd_split(coll, "mult", D, dout, saved)
        ops.emb_bwd_sgd(vw, ops.qr_virtual_bags(rows, coll, bags), gout, 0.0, ops.UPD_SORTED)

    cands = {
        "(a) dlrm_emb_fwd, fp32 tables": lambda: ops.emb_fwd(plain, bags, out),
        "(b) 2 x dlrm_emb_fwd + multiply": composed,
        "(c) dlrm_emb_fwd_qr": lambda: ops.emb_fwd_qr(Wq, Wr, rows, coll, "mult", bags, out, saved),
        "(d) plain sorted update": lambda: ops.emb_bwd_sgd(plain, bags, dout, 0.0, ops.UPD_SORTED),
        "(d) QR split + sorted update": qr_update,
    }
    for _ in range(args.warmup):
        for fn in cands.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in cands}
    for _ in range(args.repeats):
        for k, fn in cands.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    lines += ["", "### %d lookup%s per bag: %d tables (%d QR at %d collisions), D = %d, B = %d, int64 ids, rows capped at %d" %
              (hot, "" if hot == 1 else "s", T, len(qr_t), c, D, B, args.cap), "",
              "| candidate | median ms | min | max | spread (max - min) / median |", "|---|---|---|---|---|"]
    for k in cands:
        med = statistics.median(times[k])
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f %% |" % (k, med, min(times[k]), max(times[k]), 100 * (max(times[k]) - min(times[k])) / med))
    mb, mc = statistics.median(times["(b) 2 x dlrm_emb_fwd + multiply"]), statistics.median(times["(c) dlrm_emb_fwd_qr"])
    lines += ["", "(c) / (b) = %.3f; (c) / (a) = %.3f; QR update / plain update = %.3f" %
              (mc / mb, mc / statistics.median(times["(a) dlrm_emb_fwd, fp32 tables"]),
               statistics.median(times["(d) QR split + sorted update"]) / statistics.median(times["(d) plain sorted update"]))]
    del plain, Wq, Wr, cands
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cap", type=int, default=8_000_000)
    ap.add_argument("--collisions", type=int, default=4)
    ap.add_argument("--threshold", type=int, default=200)
    ap.add_argument("--hot", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_qr_emb.py measures on the GPU; none found")
    import bench
    wl = bench.WORKLOADS["criteo_terabyte"]
    D, B = wl["D"], wl["batch"]
    rows_full = [int(n) for n in wl["rows"]]
    rows = [min(n, args.cap) for n in rows_full]
    dev = torch.device("cuda:0")
    fp32, qr = table_bytes(rows_full, D, args.collisions, args.threshold)
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup), "",
             "Table bytes at the FULL Criteo-Terabyte row counts, D = %d: fp32 %.2f GB; QR at %d collisions (threshold %d) %.2f GB: %.2f GB saved (%.1f %%)" %
             (D, fp32 / 1e9, args.collisions, args.threshold, qr / 1e9, (fp32 - qr) / 1e9, 100 * (fp32 - qr) / fp32)]
    for hot in (1, args.hot):
        run(hot, rows, D, B, args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
