#!/usr/bin/env python3
"""Mixed-dimension (MD) embedding tables: the fused lookup + projection and its backward beside the composition from the kernels that existed
before, same process, same GPU, same ids.

    python tools/bench_md_emb.py [--repeats 30] [--warmup 5] [--cap 8000000] [--alpha 0.3] [--hot 4] [--out FILE.md]

Shape: the 26 Criteo-Terabyte tables of bench.py (rows capped at --cap), base D = 128, per-table widths from ops.md_solver(alpha, d0 = 128,
rounded to powers of two), B = 65536, int64 ids; once with one lookup per bag and once with --hot lookups per bag.  Timed:
  (a) forward, fused: dlrm_emb_fwd_md (writes the pooled sums for backward, as in training);
  (b) forward, composed: dlrm_emb_fwd per width group into a narrow [B, sum d] buffer (identity tables straight into their slot), then
      dlrm_linear_fwd per projected table from its columns of that buffer into its slot of the [B, T*D] output;
  (c) backward, fused: dlrm_emb_md_bwd (gradient of the pooled sums + all projection gradients, one call);
  (d) backward, composed: dlrm_linear_bwd_data + dlrm_linear_bwd_weight per projected table, a strided copy per identity table.
The sparse updates that follow are the same kernels on the same buffer in both forms and are not timed here.  If an existing kernel refuses
a shape of the composition (a width it was never built for), the table says so instead of a time.
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

import torch


def time_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(hot, rows, dims, D, B, args, dev, lines):
    from dlrm_amd import ops
    T = len(rows)
    g = torch.Generator(device=dev).manual_seed(7)
    W = [torch.empty((n, d), dtype=torch.float32, device=dev).uniform_(-0.1, 0.1, generator=g) for n, d in zip(rows, dims)]
    P = [None if d == D else torch.empty((D, d), dtype=torch.float32, device=dev).uniform_(-0.5, 0.5, generator=g) for d in dims]
    offs = [torch.arange(B, device=dev, dtype=torch.int64) * hot for _ in rows]
    idxs = [torch.randint(0, n, (B * hot,), device=dev, generator=g) for n in rows]
    bags = ops.BagBatch(offs, idxs)
    lay = ops.MDLayout(dims)
    out = torch.empty((B, T * D), dtype=torch.float32, device=dev)
    saved = torch.empty((B, lay.width), dtype=torch.float32, device=dev)
    gout = torch.empty((B, lay.width), dtype=torch.float32, device=dev)
    dout = torch.empty((B, T * D), dtype=torch.float32, device=dev).normal_(generator=g)
    dP = [None if p is None else torch.empty_like(p) for p in P]
    group_bags = [(d, ks, c0, ops.bag_subset(bags, ks)) for d, ks, c0 in lay.groups if d != D]
    ident = [t for t in range(T) if P[t] is None]
    ident_bags = [ops.bag_subset(bags, [t]) for t in ident]

    def fwd_composed():
        for d, ks, c0, gb in group_bags:
            ops.emb_fwd([W[k] for k in ks], gb, saved[:, c0:c0 + len(ks) * d])
        for t, b1 in zip(ident, ident_bags):
            ops.emb_fwd([W[t]], b1, out[:, t * D:(t + 1) * D])
        for t in range(T):
            if P[t] is not None:
                ops.linear_fwd(saved[:, lay.cols[t]:lay.cols[t] + dims[t]], P[t], None, ops.ACT_NONE, out[:, t * D:(t + 1) * D])

    def bwd_composed():
        for t in range(T):
            do = dout[:, t * D:(t + 1) * D]
            if P[t] is None:
                gout[:, lay.cols[t]:lay.cols[t] + D].copy_(do)
            else:
                ops.linear_bwd_data(do, P[t], None, ops.ACT_NONE, gout[:, lay.cols[t]:lay.cols[t] + dims[t]])
                ops.linear_bwd_weight(do, saved[:, lay.cols[t]:lay.cols[t] + dims[t]], dP[t])

    cands = {
        "(a) forward: dlrm_emb_fwd_md": lambda: ops.emb_fwd_md(W, P, D, bags, out, saved, lay.cols),
        "(b) forward: emb_fwd per width + linear_fwd per table": fwd_composed,
        "(c) backward: dlrm_emb_md_bwd": lambda: ops.emb_md_bwd(P, dims, D, dout, saved, lay.cols, gout),
        "(d) backward: linear_bwd_data + linear_bwd_weight per table": bwd_composed,
    }
    refused = {}
    for k in list(cands):
        try:
            cands[k]()
            torch.cuda.synchronize()
        except RuntimeError as e:                        # an existing kernel that does not take a shape of the composition
            refused[k] = str(e).splitlines()[0]
            del cands[k]
    for _ in range(args.warmup):
        for fn in cands.values():
            fn()
    ops.check_index_errors(sync=True)
    times = {k: [] for k in cands}
    for _ in range(args.repeats):
        for k, fn in cands.items():
            times[k].append(time_ms(fn))
    ops.check_index_errors(sync=True)
    lines += ["", "### %d lookup%s per bag: %d tables (%d projected, widths %s), D = %d, B = %d, int64 ids, rows capped at %d" %
              (hot, "" if hot == 1 else "s", T, T - len(ident), sorted(set(dims)), D, B, args.cap), "",
              "| candidate | median ms | min | max | spread (max - min) / median |", "|---|---|---|---|---|"]
    for k in cands:
        med = statistics.median(times[k])
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f %% |" % (k, med, min(times[k]), max(times[k]), 100 * (max(times[k]) - min(times[k])) / med))
    for k, why in refused.items():
        lines.append("| %s | refused: %s | | | |" % (k, why))
    med = {k[:3]: statistics.median(v) for k, v in times.items()}
    if "(a)" in med and "(b)" in med:
        lines += ["", "forward: fused / composed = %.3f" % (med["(a)"] / med["(b)"])]
    if "(c)" in med and "(d)" in med:
        lines += ["backward: fused / composed = %.3f" % (med["(c)"] / med["(d)"])]
    del W, P, cands
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cap", type=int, default=8_000_000)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--hot", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_md_emb.py measures on the GPU; none found")
    import bench
    from dlrm_amd import ops
    wl = bench.WORKLOADS["criteo_terabyte"]
    D, B = wl["D"], wl["batch"]
    rows_full = [int(n) for n in wl["rows"]]
    rows = [min(n, args.cap) for n in rows_full]
    dims = ops.md_solver(rows_full, args.alpha, d0=D, round_dim=True).tolist()
    dev = torch.device("cuda:0")
    fp32 = sum(n * D * 4 for n in rows_full)
    md = sum(n * d * 4 + (D * d * 4 if d < D else 0) for n, d in zip(rows_full, dims))
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup), "",
             "Widths from md_solver(alpha = %g, d0 = %d, rounded): %s" % (args.alpha, D, dims), "",
             "Table bytes at the FULL Criteo-Terabyte row counts: fp32 at D = %d %.2f GB; mixed widths + projections %.3f GB (%.1f %% of it)" %
             (D, fp32 / 1e9, md / 1e9, 100 * md / fp32)]
    for hot in (1, args.hot):
        run(hot, rows, dims, D, B, args, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
