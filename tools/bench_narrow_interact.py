#!/usr/bin/env python3
"""The fused narrow (D = 16 / 32 / 64) fp32 lookup + interaction kernels (forward and backward) beside the two-kernel form they replace, same
process, same GPU, same inputs.

    python tools/bench_narrow_interact.py [--rows fp32|bf16|q8|q4|qr-mult|qr-add] [--repeats 20] [--warmup 3] [--max-rows 10000000]
                                          [--out profiles/narrow_interact/fused_rates.md]

Shapes: 26 tables, one lookup per bag, int64 ids; D = 64 with the Criteo-Terabyte row counts and D = 16 with the Criteo-Kaggle row counts
(bench.py WORKLOADS), each at B = 2048 and B = 65536; row counts capped at --max-rows per table.
  forward : dlrm_interact_fwd_gather_narrow (fused);  dlrm_emb_fwd + dlrm_interact_fwd over the buffer the lookup wrote (both launches inside
            one timed interval, and the lookup alone).
  backward: dlrm_interact_bwd_gather_narrow (fused);  dlrm_interact_bwd over (x, the pooled buffer) — the backward of the two-kernel form.

Protocol (docs/MEASUREMENT.md): warm-up rounds, then `repeats` rounds; every round times each variant once between two HIP events (the
variants alternate inside a round, so drift hits all alike); the MEDIAN over the rounds is reported with min / max.  Before timing, the
fused results are compared with the two-kernel results bit for bit.  Algorithmic bytes: ids + offsets, table row bytes, x, R / dR, dx and
dE; the two-kernel form adds the [B, T*D] fp32 buffer (forward: written and read back; backward: read).  No GPU: the tool fails.

--rows bf16 | q8 | q4 (default fp32, whose output is unchanged): the same shapes over bfloat16 tables (dlrm_interact_{fwd,bwd}_gather_narrow_bf16
against dlrm_emb_fwd_bf16 + the generic interaction kernels) or over 8- / 4-bit packed tables (dlrm_interact_fwd_gather_narrow_quant against
dlrm_emb_fwd_quant + dlrm_interact_fwd; forward only: there is no backward over packed tables).  The table bytes of a lookup are then
2 D, D + 8 and D/2 + 4 per row.

--rows qr-mult | qr-add: the same shapes over quotient-remainder tables — a table is QR with the reference's defaults (--qr-collisions 4,
--qr-threshold 200) where its row count exceeds the threshold, plain fp32 otherwise.  Forward: dlrm_interact_fwd_gather_narrow_qr against
dlrm_emb_fwd_qr (saving the two pooled sums for "mult", as a training forward does) + dlrm_interact_fwd, and the lookup alone.  Backward:
dlrm_interact_bwd_gather_narrow_qr against dlrm_interact_bwd + dlrm_emb_qr_bwd_split.  Algorithmic bytes: a QR lookup reads a weight_q and a
weight_r row; the two-kernel form writes the [B, 2*Tq*D] sums in the forward and reads them in the backward, where it also writes and reads
the [B, T*D] gradient of the pooled buffer in front of the [B, Tv*D] buffer of the virtual table list; the fused "mult" backward reads the
ids, both rows and the q slots a second time (its in-place multiplication)."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ROW_KINDS = ("fp32", "bf16", "q8", "q4", "qr-mult", "qr-add")
QR_COLLISIONS, QR_THRESHOLD = 4, 200          # the reference's --qr-collisions / --qr-threshold defaults
# per row kind: the suffix of the fused entry points, the lookup of the two-kernel form
_SUFFIX = {"fp32": "", "bf16": "_bf16", "q8": "_quant", "q4": "_quant"}
_LOOKUP = {"fp32": "dlrm_emb_fwd", "bf16": "dlrm_emb_fwd_bf16", "q8": "dlrm_emb_fwd_quant", "q4": "dlrm_emb_fwd_quant"}


def labels(kind):
    if kind.startswith("qr"):
        return ("forward: fused (dlrm_interact_fwd_gather_narrow_qr)", "forward: two kernels (dlrm_emb_fwd_qr + dlrm_interact_fwd)",
                "forward: lookup alone (dlrm_emb_fwd_qr)", "backward: fused (dlrm_interact_bwd_gather_narrow_qr)",
                "backward: two-kernel form (dlrm_interact_bwd + dlrm_emb_qr_bwd_split)")
    return ("forward: fused (dlrm_interact_fwd_gather_narrow%s)" % _SUFFIX[kind],
            "forward: two kernels (%s + dlrm_interact_fwd)" % _LOOKUP[kind],
            "forward: lookup alone (%s)" % _LOOKUP[kind],
            "backward: fused (dlrm_interact_bwd_gather_narrow%s)" % _SUFFIX[kind],
            "backward: two-kernel form (dlrm_interact_bwd)")


def row_bytes(kind, D):
    return {"fp32": 4 * D, "bf16": 2 * D, "q8": D + 8, "q4": D // 2 + 4, "qr-mult": 4 * D, "qr-add": 4 * D}[kind]      # (qr: per component row)


def time_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def same_bits(a, b) -> bool:
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def make_tables(rows, D, dev, g, kind="fp32"):
    from dlrm_amd import ops
    out = []
    for n in rows:
        w = torch.empty((n, D), dtype=torch.float32, device=dev).uniform_(-float(n) ** -0.5, float(n) ** -0.5, generator=g)
        if kind == "bf16":
            w = w.to(torch.bfloat16)
        elif kind != "fp32":
            w = ops.emb_quantize(w, 8 if kind == "q8" else 4)
        out.append(w)
    return out


def make_qr_tables(rows, D, dev, g):
    """(weight_q or plain weight, weight_r or None, categories, collisions) per table"""
    W, Wr, coll = [], [], []
    for n in rows:
        c = QR_COLLISIONS if n > QR_THRESHOLD else 0
        nq = -(-n // c) if c else n
        W.append(torch.empty((nq, D), dtype=torch.float32, device=dev).uniform_(-float(n) ** -0.5, float(n) ** -0.5, generator=g))
        Wr.append(torch.empty((c, D), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=g) if c else None)
        coll.append(c)
    return W, Wr, list(rows), coll


def run_shape(name, tables, D, B, args, dev, lines, g):
    from dlrm_amd import ops
    kind = args.rows
    FWD_FUSED, FWD_TWO, FWD_LOOKUP, BWD_FUSED, BWD_TWO = labels(kind)
    qr = kind.startswith("qr")
    if qr:
        tables, tables_r, rows, coll = tables
        op, Tq = kind[3:], sum(1 for c in coll if c)
    else:
        rows = [w.size(0) for w in tables]
    T = len(rows)
    F = T + 1
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
    R = {k: torch.empty((B, ldr), dtype=torch.float32, device=dev) for k in ("fused", "two")}
    G = {k: (torch.empty((B, D), dtype=torch.float32, device=dev),
             torch.empty((B, (T + Tq if qr else T) * D), dtype=torch.float32, device=dev)) for k in ("fused", "two")}
    mode = ops.INTERACT_RELU_X          # what the model's backward passes (the bottom tower ends in a ReLU)

    bits = {"q8": 8, "q4": 4}.get(kind)
    if kind == "fp32":
        lookup = lambda: ops.emb_fwd(tables, bags, E)
        fused_fwd = lambda: ops.interact_fwd_gather_narrow(x, tables, bags, D, 0, R["fused"])
        fused_bwd = lambda: ops.interact_bwd_gather_narrow(x, tables, bags, D, mode, dR, *G["fused"])
    elif kind == "bf16":
        lookup = lambda: ops.emb_fwd_bf16(tables, bags, E)
        fused_fwd = lambda: ops.interact_fwd_gather_narrow_bf16(x, tables, bags, D, 0, R["fused"])
        fused_bwd = lambda: ops.interact_bwd_gather_narrow_bf16(x, tables, bags, D, mode, dR, *G["fused"])
    elif qr:
        saved = torch.empty((B, 2 * Tq * D), dtype=torch.float32, device=dev) if op == "mult" else None
        dE = torch.empty((B, T * D), dtype=torch.float32, device=dev)
        lookup = lambda: ops.emb_fwd_qr(tables, tables_r, rows, coll, op, bags, E, saved)
        fused_fwd = lambda: ops.interact_fwd_gather_narrow_qr(x, tables, tables_r, rows, coll, op, bags, D, 0, R["fused"])
        fused_bwd = lambda: ops.interact_bwd_gather_narrow_qr(x, tables, tables_r, rows, coll, op, bags, D, mode, dR, *G["fused"])

        def two_bwd():
            ops.interact_bwd((x, E), D, mode, dR, (G["two"][0], dE))
            ops.emb_qr_bwd_split(coll, op, D, dE, saved, G["two"][1])
    else:
        lookup = lambda: ops.emb_fwd_quant(tables, rows, D, bits, bags, E)
        fused_fwd = lambda: ops.interact_fwd_gather_narrow_quant(x, tables, rows, D, bits, bags, 0, R["fused"])
        fused_bwd = None                      # packed tables are constants: forward only

    def two_fwd():
        lookup()
        ops.interact_fwd((feat,), D, 0, R["two"])
    kernels = {FWD_FUSED: fused_fwd, FWD_TWO: two_fwd, FWD_LOOKUP: lookup}
    if fused_bwd is not None:
        kernels[BWD_FUSED] = fused_bwd
        kernels[BWD_TWO] = two_bwd if qr else (lambda: ops.interact_bwd((x, E), D, mode, dR, G["two"]))
    # the results the timed kernels compute are the same bits
    for fn in kernels.values():
        fn()
    ops.check_index_errors(sync=True)
    if not same_bits(R["fused"], R["two"]) or (fused_bwd is not None and (not same_bits(G["fused"][0], G["two"][0])
                                                                         or not same_bits(G["fused"][1], G["two"][1]))):
        sys.exit("ERROR: %s: the fused narrow kernels and the two-kernel form differ" % name)
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
    trow = B * T * row_bytes(kind, D)         # the table rows read (fp32 rows: as many bytes as the buffer)
    total = {
        FWD_FUSED: sel + trow + xb + rb,
        FWD_TWO: sel + trow + 2 * buf + xb + rb,
        FWD_LOOKUP: sel + trow + buf,
        BWD_FUSED: sel + trow + xb + rb + grads,
        BWD_TWO: buf + xb + rb + grads,
    }
    if qr:
        trow = B * sum((2 if c else 1) * 4 * D for c in coll)          # a QR lookup reads a weight_q and a weight_r row
        sums = B * 2 * Tq * D * 4 if op == "mult" else 0               # the pooled sums the two-kernel forward keeps
        gout = B * (T + Tq) * D * 4
        again = (B * Tq * 8 + B * Tq * 2 * 4 * D + B * Tq * D * 4) if op == "mult" else 0      # the in-place multiplication: ids, both rows, the q slots
        total = {
            FWD_FUSED: sel + trow + xb + rb,
            FWD_TWO: sel + trow + 2 * buf + sums + xb + rb,
            FWD_LOOKUP: sel + trow + buf + sums,
            BWD_FUSED: sel + trow + xb + rb + xb + gout + again,
            BWD_TWO: buf + xb + rb + xb + 2 * buf + sums + gout,
        }
    lines.append("")
    lines.append("### %s: %d tables (%.1f M rows, at most %d per table), D = %d, B = %d, one lookup per bag, int64 ids%s" %
                 (name, T, sum(rows) / 1e6, max(rows), D, B, "" if kind == "fp32" else ", %s rows" % kind)
                 + (" (%d QR tables, %d collisions)" % (Tq, QR_COLLISIONS) if qr else ""))
    lines.append("")
    lines.append("| kernel | median ms | min | max | algorithmic MB | GB/s |")
    lines.append("|---|---|---|---|---|---|")
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        lines.append("| %s | %.4f | %.4f | %.4f | %.1f | %.0f |" % (k, med[k], min(ts), max(ts), total[k] / 1e6, total[k] / med[k] / 1e6))
    lines.append("")
    pairs = [("forward", FWD_FUSED, FWD_TWO)] + ([("backward", BWD_FUSED, BWD_TWO)] if fused_bwd is not None else [])
    for what, f, t in ((w, med[a], med[b]) for w, a, b in pairs):
        lines.append("%s: fused %.4f ms, two-kernel form %.4f ms (fused is %.2fx %s)" %
                     (what, f, t, t / f if f <= t else f / t, "faster" if f < t else "SLOWER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=10_000_000, help="cap of every table's row count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", choices=ROW_KINDS, default="fp32", help="row kind of the tables: fp32 (default), bfloat16, 8- or 4-bit packed, quotient-remainder with --qr-operation mult / add")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ERROR: tools/bench_narrow_interact.py measures on the GPU; none found")
    import bench
    dev = torch.device("cuda:0")
    lines = ["GPU: %s; torch %s; %d repeats after %d warm-up rounds, HIP events, median; all kernels in one process, alternating inside every round%s" %
             (torch.cuda.get_device_name(0), torch.__version__, args.repeats, args.warmup, "" if args.rows == "fp32" else "; %s tables" % args.rows)]
    g = torch.Generator(device=dev).manual_seed(7)
    for workload, D in (("criteo_terabyte", 64), ("criteo_kaggle", 16)):
        capped = [min(n, args.max_rows) for n in bench.WORKLOADS[workload]["rows"]]
        tables = make_qr_tables(capped, D, dev, g) if args.rows.startswith("qr") else make_tables(capped, D, dev, g, args.rows)
        for B in (2048, 65536):
            run_shape("%s rows" % workload, tables, D, B, args, dev, lines, g)
        del tables
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
