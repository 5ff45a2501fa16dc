"""Bits of the interaction launches, the tower kernels and a training step: runs the calls of tests/test_gpu_interact_dispatch.py (every
dispatched NI / NB, with and without predicate, the update inside the backward, the dynamic-LDS sequences) with whatever library
DLRM_HIP_LIB names and prints, per test case, one SHA-256 over every tensor those calls wrote (name, dtype, shape and bytes, in call order);
then bench.py's default model for two steps, hashed from its --dump-outputs files (loss, model output, dense parameters, table rows) —
once with the default sparse update (DLRM_UPD_SORTED: the partial sums of a hot row meet in fp32 atomics, whose order is the hardware's)
and once with --emb-update deterministic, which has no atomics.

    DLRM_HIP_LIB=<parent build> python tools/interact_dispatch_identity.py --out A.json       # one column
    python tools/interact_dispatch_identity.py --table --parent A.json B.json C.json --new D.json E.json   # -> profiles/interact_dispatch/identity.md

A cell is stable when all parent columns agree and all new columns agree; the table fails (exit 1) if a stable cell differs between parent
and new, or if an unstable cell has no value that both a parent and a new column show.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# what each call writes: positions in its argument list as the test file calls it ("ret.mask": a field of the returned object)
WRITES = {
    "interact_fwd": (3,), "interact_bwd": (4,), "emb_fwd": (2,),
    "interact_fwd_gather": (5,), "interact_bwd_gather": (6, 7, 1),        # dx, dE and (update inside the backward) the tables
    "emb_presort": ("ret.mask",), "emb_bwd_sgd": (0,), "emb_bwd_sgd_presorted": (0,),
    "tower_fwd": (4,), "tower_bwd": (4, 5),
}


class Recorder:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, name, t):
        import torch
        if t is None:
            return
        if isinstance(t, (list, tuple)):
            for i, u in enumerate(t):
                self.add("%s[%d]" % (name, i), u)
            return
        t = t.detach().contiguous().cpu()
        self.h.update(("%s %s %s;" % (name, t.dtype, tuple(t.shape))).encode())
        self.h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())

    def wrap(self, name, fn):
        def call(*a, **k):
            ret = fn(*a, **k)
            for w in WRITES[name]:
                self.add("%s.%s" % (name, w), ret.mask if w == "ret.mask" else a[w])
            return ret
        return call


def run_cell(fn):
    import pytest
    from dlrm_amd import ops
    rec = Recorder()
    with pytest.MonkeyPatch.context() as mp:
        for name in WRITES:
            mp.setattr(ops, name, rec.wrap(name, getattr(ops, name)))
        fn()
    return rec.h.hexdigest()


def bench_cells(update):
    """bench.py --gpus 1 (default workload), one warm-up step and two timed ones, in a process of its own: the files of --dump-outputs"""
    import numpy as np
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--emb-update", update,
                            "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("bench.py failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        groups = {"loss": [], "model output": [], "tower parameters": [], "table rows": []}
        for f in sorted(os.listdir(d)):
            g = "loss" if f == "loss.npy" else "model output" if f == "Z.npy" else "table rows" if f.startswith("emb_l.") else "tower parameters"
            groups[g].append(f)
        out = {}
        for g, files in groups.items():
            h = hashlib.sha256()
            for f in files:
                a = np.load(os.path.join(d, f))
                h.update(("%s %s %s;" % (f, a.dtype, a.shape)).encode())
                h.update(np.ascontiguousarray(a).tobytes())
            out["bench.py --gpus 1, 2 steps|update %s|%s (%d files)" % (update, g, len(files))] = h.hexdigest()
        return out


def digests():
    import torch
    import test_gpu_interact_dispatch as T
    out = {}
    for F in T.PLAIN_F:
        out["plain|D128|F%d" % F] = run_cell(lambda: T.test_every_ni_of_the_plain_image_kernels(F))
    for F in T.GATHER_F:
        for dt in (torch.int32, torch.int64):
            out["gather|D128|F%d|%s" % (F, str(dt)[6:])] = run_cell(lambda: T.test_every_ni_of_the_gather_image_kernels(F, dt))
    for F in T.UPDATE_F:
        out["update_in_backward|D128|F%d" % F] = run_cell(lambda: T.test_update_inside_the_backward_at_both_ends_of_ni(F))
    for F, D in T.GENERIC_SHAPES:
        out["generic|D%d|F%d" % (D, F)] = run_cell(lambda: T.test_generic_kernels_with_and_without_a_predicate(F, D))
    out["lds_limit_sequences"] = run_cell(T.lds_limit_sequences)
    torch.cuda.synchronize()
    out.update(bench_cells("sorted"))
    out.update(bench_cells("deterministic"))
    return out


def table(parents, news):
    P, N = [json.load(open(f)) for f in parents], [json.load(open(f)) for f in news]
    keys = list(P[0])
    assert all(list(d) == keys for d in P + N)
    head = ["parent %d" % (i + 1) for i in range(len(P))] + ["new %d" % (i + 1) for i in range(len(N))]
    print("| case | %s |\n|---|%s" % (" | ".join(head), "---|" * len(head)))
    unstable, differ, foreign = [], [], []
    for k in keys:
        pv, nv = {d[k] for d in P}, {d[k] for d in N}
        print("| `%s` | %s |" % (k.replace("|", " / "), " | ".join(d[k][:16] for d in P + N)))
        if len(pv) > 1 or len(nv) > 1:
            unstable.append(k)
            if not nv & pv:
                foreign.append(k)
        elif pv != nv:
            differ.append(k)
    lines = lambda ks: "".join("\n- `%s`" % k for k in ks)
    print("\n%d cases, %d parent and %d new columns; %d not reproduced by a library against itself%s; of those, %d where no new column shows a "
          "parent's value%s; %d of the stable ones differ between parent and new%s."
          % (len(keys), len(P), len(N), len(unstable), lines(unstable), len(foreign), lines(foreign), len(differ), lines(differ)))
    return 1 if differ or foreign else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--new", nargs="+")
    args = ap.parse_args()
    if args.table:
        sys.exit(table(args.parent, args.new))
    d = digests()
    with open(args.out, "w") as f:
        json.dump(d, f, indent=0)
        f.write("\n")
    print("%d cases -> %s" % (len(d), args.out))
