"""Bits of the two-kernel embedding path and the sparse update behind it: runs the cases of tests/test_gpu_emb_update.py in THIS checkout and
prints, per case, one SHA-256 over the losses, every parameter and every optimizer state tensor after the case's two steps (name and bytes of
each, in order).

    python tools/emb_update_identity.py --out A.json                 # one column
    python tools/emb_update_identity.py --table A.json B.json C.json # parent, parent again, new -> the markdown of profiles/emb_update/identity.md
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digests():
    import pytest
    import torch
    import test_gpu_emb_update as U
    out = {}
    for case in U.cases():
        with pytest.MonkeyPatch.context() as mp:
            _, tensors = U.run_case(case, mp)
        h = hashlib.sha256()
        for name, t in tensors.items():
            t = t.detach()
            if t.is_sparse:                                    # (SGD's momentum buffer of a COO gradient)
                t = t.coalesce()
                t = torch.cat([t.indices().reshape(-1).double(), t.values().reshape(-1).double()])
            t = t.contiguous().cpu()
            h.update(("%s %s %s;" % (name, t.dtype, tuple(t.shape))).encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        out[U.case_id(case)] = h.hexdigest()
    return out


def table(parent_a, parent_b, new):
    a, b, c = (json.load(open(f)) for f in (parent_a, parent_b, new))
    assert list(a) == list(b) == list(c)
    unstable = [k for k in a if a[k] != b[k]]
    differ = [k for k in a if a[k] == b[k] and a[k] != c[k]]
    print("| case | parent | parent again | new |\n|---|---|---|---|")
    for k in a:
        print("| `%s` | %s | %s | %s |" % (k, a[k][:16], b[k][:16], c[k][:16]))
    print("\n%d cases; %d the parent does not reproduce against itself%s; %d of the others differ in the new tree%s."
          % (len(a), len(unstable), "".join("\n- `%s`" % k for k in unstable), len(differ), "".join("\n- `%s`" % k for k in differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--table", nargs=3)
    args = ap.parse_args()
    if args.table:
        sys.exit(table(*args.table))
    d = digests()
    with open(args.out, "w") as f:
        json.dump(d, f, indent=0)
        f.write("\n")
    print("%d cases -> %s" % (len(d), args.out))
