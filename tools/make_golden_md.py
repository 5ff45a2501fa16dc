#!/usr/bin/env python3
"""Write tests/golden/md_training.npz by RUNNING THE REFERENCE's mixed-dimension (MD) embedding training on the CPU.

    DLRM_REFERENCE=<checkout of facebookresearch/dlrm> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_md.py

The reference's `DLRM_Net` is imported as a library (as oracle/make_golden.py does) and built with `md_flag=True` after
`np.random.seed(seed)` and `torch.manual_seed(seed)` — the projections are drawn from torch's generator, the tables from numpy's.  The
per-table dimensions of case "pow2" come from the reference's own `md_solver` (as run() calls it, dlrm_s_pytorch.py:1213-1219); the other
cases hand dimensions to `DLRM_Net` directly ("odd": what --md-round-dims false can produce).  md_threshold lies below the smallest table:
the reference cannot build a table at or below it under md_flag.  Each case trains STEPS steps of plain SGD (zero_grad / backward / step,
sparse embedding gradients) on fixed batches.  The fixture holds data only: per case the dimensions, the initial parameters (`init.`), the
inputs, the loss and the predictions of every step, and the final parameters (`final.`).
tests/test_md_emb_host.py pins the fixture to torch's operators and to this project's initialisation on the CPU;
tests/test_gpu_md_emb.py trains this project's model on the device from the same parameters.
"""
from __future__ import annotations

import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

STEPS, LR = 3, 0.1
TABLES = [60, 3, 500, 1200, 250]
CASES = {
    "pow2": dict(d0=16, ln_emb=TABLES, ln_bot=[13, 32, 16], batch=64, max_len=4, dims=None, alpha=0.3, round_dims=True, seed=41),
    "odd": dict(d0=16, ln_emb=TABLES, ln_bot=[13, 32, 16], batch=64, max_len=4, dims=[16, 3, 12, 1, 6], seed=42),
    "onehot128": dict(d0=128, ln_emb=[260, 3, 401], ln_bot=[13, 64, 128], batch=48, max_len=0, dims=[32, 128, 8], seed=43),
}
THRESHOLD = 2


def main() -> None:
    if not os.environ.get("DLRM_REFERENCE"):
        sys.exit("set DLRM_REFERENCE to a checkout of the reference (facebookresearch/dlrm)")
    import make_golden                                   # (reads DLRM_REFERENCE; stubs torch.utils.tensorboard)
    ref, _dp, _ext = make_golden.import_reference()
    out, meta = {}, {"steps": STEPS, "lr": LR, "md_threshold": THRESHOLD, "torch": torch.__version__, "cases": {}}
    for name, c in CASES.items():
        F = len(c["ln_emb"]) + 1
        ln_top = [c["d0"] + F * (F - 1) // 2, 32, 1]
        if c["dims"] is None:
            m_spa = ref.md_solver(torch.tensor(c["ln_emb"]), c["alpha"], d0=c["d0"], round_dim=c["round_dims"]).tolist()
        else:
            m_spa = list(c["dims"])
        print(name, "m_spa as the reference has it:", m_spa)
        out[f"{name}.dims"] = np.asarray(m_spa, dtype=np.float64)
        m_spa = [int(d) for d in m_spa]
        np.random.seed(c["seed"])
        torch.manual_seed(c["seed"])
        model = ref.DLRM_Net(m_spa, np.asarray(c["ln_emb"]), np.asarray(c["ln_bot"]), np.asarray(ln_top), arch_interaction_op="dot",
                             sigmoid_top=len(ln_top) - 2, loss_function="bce", md_flag=True, md_threshold=THRESHOLD)
        for k, v in model.state_dict().items():
            out[f"{name}.init.{k}"] = v.numpy().copy()
        opt = torch.optim.SGD(model.parameters(), lr=LR)
        rng = np.random.default_rng(c["seed"])
        B = c["batch"]
        for s in range(STEPS):
            X = rng.random((B, c["ln_bot"][0])).astype(np.float32)
            T = np.round(rng.random((B, 1))).astype(np.float32)
            lS_o, lS_i = [], []
            for n in c["ln_emb"]:
                lens = rng.integers(0, c["max_len"] + 1, size=B) if c["max_len"] else np.ones(B, dtype=np.int64)
                lS_o.append(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
                lS_i.append(rng.integers(0, n, size=int(lens.sum())).astype(np.int64))
            Z = model(torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i])
            E = model.loss_fn(Z, torch.from_numpy(T))
            opt.zero_grad()
            E.backward()
            opt.step()
            out[f"{name}.s{s}.X"], out[f"{name}.s{s}.T"] = X, T
            for k in range(len(c["ln_emb"])):
                out[f"{name}.s{s}.off{k}"], out[f"{name}.s{s}.idx{k}"] = lS_o[k], lS_i[k]
            out[f"{name}.s{s}.loss"] = np.asarray(E.item(), dtype=np.float32)
            out[f"{name}.s{s}.pred"] = Z.detach().numpy().copy()
        for k, v in model.state_dict().items():
            out[f"{name}.final.{k}"] = v.numpy().copy()
        meta["cases"][name] = dict(c, dims=m_spa, ln_top=ln_top, sigmoid_top=len(ln_top) - 2)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "md_training.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
