#!/usr/bin/env python3
"""Write tests/golden/qr_training.npz by RUNNING THE REFERENCE's quotient-remainder (QR) embedding training on the CPU.

    DLRM_REFERENCE=<checkout of facebookresearch/dlrm> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_qr.py

The reference's `DLRM_Net` is imported as a library (as oracle/make_golden.py does) and built with `qr_flag=True` after
`np.random.seed(seed)` and `torch.manual_seed(seed)` — QR tables are drawn from torch's generator, the other parameters from numpy's.
Each case trains STEPS steps of plain SGD (zero_grad / backward / step, sparse embedding gradients) on fixed batches.  The reference draws
QR tables U(sqrt(1 / n), 1): with multi-hot bags the pooled products saturate the sigmoid at once (losses above 20, predictions of exactly 0
or 1), which tests nothing — so training STARTS from the initial parameters with the QR tables multiplied by the case's `qr_scale`.  The
fixture holds data only: per case the initial parameters as constructed (`init.`), the parameters training starts from (`start.`), the
inputs, the loss and the predictions of every step, and the final parameters (`final.`).
tests/test_qr_emb_host.py pins the fixture to torch's operators and to this project's initialisation on the CPU;
tests/test_gpu_qr_emb.py trains this project's model on the device from the same parameters.
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
# threshold 200: three of the five tables are QR; 250 and 500 rows leave a ragged last quotient row at 4 and 7 collisions (and at 4: 1200 does not)
CASES = {
    "mult": dict(m_spa=16, ln_emb=[60, 3, 500, 1200, 250], ln_bot=[13, 32, 16], batch=64, max_len=4, op="mult", collisions=4, seed=31, qr_scale=0.25),
    "add": dict(m_spa=16, ln_emb=[60, 3, 500, 1200, 250], ln_bot=[13, 32, 16], batch=64, max_len=4, op="add", collisions=7, seed=32, qr_scale=0.125),
    "onehot128": dict(m_spa=128, ln_emb=[260, 3, 401], ln_bot=[13, 64, 128], batch=48, max_len=0, op="mult", collisions=4, seed=33, qr_scale=1.0),
}
THRESHOLD = 200


def main() -> None:
    if not os.environ.get("DLRM_REFERENCE"):
        sys.exit("set DLRM_REFERENCE to a checkout of the reference (facebookresearch/dlrm)")
    import make_golden                                   # (reads DLRM_REFERENCE; stubs torch.utils.tensorboard)
    ref, _dp, _ext = make_golden.import_reference()
    out, meta = {}, {"steps": STEPS, "lr": LR, "qr_threshold": THRESHOLD, "torch": torch.__version__, "cases": {}}
    for name, c in CASES.items():
        F = len(c["ln_emb"]) + 1
        ln_top = [c["m_spa"] + F * (F - 1) // 2, 32, 1]
        np.random.seed(c["seed"])
        torch.manual_seed(c["seed"])
        model = ref.DLRM_Net(c["m_spa"], np.asarray(c["ln_emb"]), np.asarray(c["ln_bot"]), np.asarray(ln_top), arch_interaction_op="dot",
                             sigmoid_top=len(ln_top) - 2, loss_function="bce", qr_flag=True, qr_operation=c["op"],
                             qr_collisions=c["collisions"], qr_threshold=THRESHOLD)
        for k, v in model.state_dict().items():
            out[f"{name}.init.{k}"] = v.numpy().copy()
        with torch.no_grad():
            for k, p in model.named_parameters():
                if k.endswith((".weight_q", ".weight_r")):
                    p.mul_(c["qr_scale"])
        for k, v in model.state_dict().items():
            out[f"{name}.start.{k}"] = v.numpy().copy()
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
        meta["cases"][name] = dict(c, ln_top=ln_top, sigmoid_top=len(ln_top) - 2)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "qr_training.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
