#!/usr/bin/env python3
"""Time of one exact sparse Adagrad update of the embedding tables, three ways, same process, same GPU, same inputs.

    python tools/bench_adagrad_emb.py [--repeats 20] [--warmup 3] [--cap 8000000] [--out FILE.md]

Shape: the 26 Criteo-Terabyte tables of bench.py (rows capped at --cap so that three sets of tables and their accumulators fit side by
side), D = 128, B = 65536, one lookup per bag, int64 ids.  The three updates:
  COO route   what torch.optim.Adagrad costs without the fused kernel (DLRM_Net.fused_adagrad = False): ops.emb_bwd_coo writes the
              [lookups, D] COO values, torch.sparse_coo_tensor wraps them per table, torch.optim.Adagrad.step coalesces and updates
  exact       dlrm_emb_bwd_adagrad (ops.emb_bwd_adagrad): [rows, D] accumulators, no COO buffer
  row-wise    dlrm_emb_bwd_rowwise_adagrad (ops.emb_bwd_rowwise_adagrad): [rows] accumulators — a different optimizer, for scale

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each update once between two HIP events (the
updates alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported, with min / max.  The fused kernels
include their sort.  A measurement path that finds no GPU fails."""
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


def run(wl, args, dev, lines):
    from dlrm_amd import ops
    D, B = wl["D"], wl["batch"]
    rows = [min(int(n), args.cap) for n in wl["rows"]]
    T = len(rows)
    lr, eps, acc0 = 1e-3, 1e-10, 0.01
    g = torch.Generator(device=dev).manual_seed(7)

    def tables():
        out = []
        for n in rows:
            bound = float(np.sqrt(1.0 / n))
            out.append(torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-bound, bound, generator=g))
        return out

    w_coo = [torch.nn.Parameter(w) for w in tables()]
    opt = torch.optim.Adagrad(w_coo, lr=lr, initial_accumulator_value=acc0, eps=eps)
    w_exact, w_rws = tables(), tables()
    sums = [torch.full((n, D), acc0, dtype=torch.float32, device=dev) for n in rows]
    moms = [torch.full((n,), acc0, dtype=torch.float32, device=dev) for n in rows]
    offs = [torch.arange(B, device=dev, dtype=torch.int64) for _ in rows]
    idxs = [torch.randint(0, n, (B,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    dout = torch.empty((B, T * D), dtype=torch.float32, device=dev).uniform_(-1e-3, 1e-3, generator=g)

    def coo_route():
        # (DLRM_Net._materialize_coo_grads without its host-side index check, then the optimizer's own step)
        values = ops.emb_bwd_coo(bags, dout, D)
        for k, (w, v) in enumerate(zip(w_coo, values)):
            w.grad = torch.sparse_coo_tensor(ops.bag_index_tensor(bags, k).reshape(1, -1).long(), v, size=tuple(w.shape),
                                             check_invariants=False)
        opt.step()

    updates = {
        "COO route: emb_bwd_coo + sparse_coo_tensor + torch.optim.Adagrad.step": coo_route,
        "dlrm_emb_bwd_adagrad (exact, fused)": lambda: ops.emb_bwd_adagrad(w_exact, sums, bags, dout, lr, eps),
        "dlrm_emb_bwd_rowwise_adagrad (row-wise, fused)": lambda: ops.emb_bwd_rowwise_adagrad(w_rws, moms, bags, dout, lr, eps),
    }
    for _ in range(args.warmup):
        for fn in updates.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in updates}
    for _ in range(args.repeats):
        for k, fn in updates.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    lines.append("")
    lines.append("### criteo_terabyte: %d tables (rows capped at %d), D = %d, B = %d, one lookup per bag, int64 ids, %.1f GB of fp32 tables per set" %
                 (T, args.cap, D, B, sum(rows) * D * 4 / 1e9))
    lines.append("")
    lines.append("| update of all tables | median ms | min | max | vs COO route |")
    lines.append("|---|---|---|---|---|")
    base = None
    for k in updates:
        med = statistics.median(times[k])
        base = med if base is None else base
        lines.append("| %s | %.4f | %.4f | %.4f | %.2fx |" % (k, med, min(times[k]), max(times[k]), base / med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=8_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_adagrad_emb.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup)]
    run(bench.WORKLOADS["criteo_terabyte"], args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
