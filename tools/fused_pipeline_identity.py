"""Bits of the fused lookup + interaction kernels AND of the two-kernel form they are tested against: runs every case of the forward and
backward bit-identity grids of the six fused-kernel test files (tests/test_gpu_{bf16,quant,qr}_interact.py, test_gpu_narrow_interact.py,
test_gpu_narrow_rows.py, test_gpu_narrow_qr.py) with whatever library DLRM_HIP_LIB names and prints, per case, one SHA-256 over every tensor
argument of every `ops.interact_*` / `ops.emb_fwd*` call the case makes (name, dtype, shape and bytes, after the call, in call order; torch's
generator is seeded per case) — so
a change that moved the fused kernels and interact.hip's kernels TOGETHER, which the tests cannot see, shows here against the parent's
library.  Then bench.py's default model for two steps with --emb-update deterministic, as tools/interact_dispatch_identity.py hashes it.

    DLRM_HIP_LIB=<parent build> python tools/fused_pipeline_identity.py --out A.json       # one column
    python tools/fused_pipeline_identity.py --table --parent A.json B.json C.json --new D.json E.json F.json   # -> profiles/fused_pipeline/identity.md

The table and its verdict are interact_dispatch_identity.py's.
"""
import argparse
import importlib
import itertools
import json
import sys

import interact_dispatch_identity as base      # (puts the repository and tests/ on sys.path)

MODULES = ("test_gpu_bf16_interact", "test_gpu_quant_interact", "test_gpu_qr_interact", "test_gpu_narrow_interact", "test_gpu_narrow_rows",
           "test_gpu_narrow_qr")
GRIDS = ("test_forward_bit_identity_grid", "test_backward_bit_identity_grid", "test_bit_identity_grid")


def cases(fn):
    """(id, kwargs) of every case of a parametrised test, from its pytest marks"""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            names = [n.strip() for n in m.args[0].split(",")]
            axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    for combo in itertools.product(*reversed(axes)):
        kw = {k: v for d in combo for k, v in d.items()}
        yield "/".join("%s=%s" % (k, str(v).replace("torch.", "")) for k, v in kw.items()), kw


def run_cell(fn, kw):
    import pytest
    import torch
    from dlrm_amd import ops
    rec = base.Recorder()

    def wrap(name, f):
        def call(*a, **k):
            ret = f(*a, **k)
            for i, t in enumerate(a):
                if isinstance(t, torch.Tensor) or (isinstance(t, (list, tuple)) and t and all(isinstance(u, torch.Tensor) for u in t)):
                    rec.add("%s.%d" % (name, i), t)
            return ret
        return call

    torch.manual_seed(2024)          # the grids draw x and dR from torch's global generator
    with pytest.MonkeyPatch.context() as mp:
        for name in dir(ops):
            if (name.startswith("interact_fwd") or name.startswith("interact_bwd") or name.startswith("emb_fwd")) and callable(getattr(ops, name)):
                mp.setattr(ops, name, wrap(name, getattr(ops, name)))
        fn(**kw)
    return rec.h.hexdigest()


def digests(only=None, bench=True):
    import torch
    out = {}
    for mod in MODULES:
        if only and only not in mod:
            continue
        T = importlib.import_module(mod)
        for g in GRIDS:
            fn = getattr(T, g, None)
            if fn is None:
                continue
            for cid, kw in cases(fn):
                out["%s|%s|%s" % (mod[9:], g[5:], cid)] = run_cell(fn, kw)
    torch.cuda.synchronize()
    if bench:
        out.update(base.bench_cells("deterministic"))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--new", nargs="+")
    ap.add_argument("--only", help="test modules whose name contains this, without the bench.py step (a quick look)")
    args = ap.parse_args()
    if args.table:
        sys.exit(base.table(args.parent, args.new))
    d = digests(args.only, not args.only)
    with open(args.out, "w") as f:
        json.dump(d, f, indent=0)
        f.write("\n")
    print("%d cases -> %s" % (len(d), args.out))
