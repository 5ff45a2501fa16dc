#!/usr/bin/env python3
"""Write tests/golden/quant_inference.npz by RUNNING THE REFERENCE's quantised inference on the CPU.

    DLRM_REFERENCE=<checkout of facebookresearch/dlrm> PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_quant.py

The reference's `DLRM_Net` is imported as a library (as oracle/make_golden.py does), built from a fixed numpy seed, and for bits in
(4, 8) a fresh copy of it calls `quantize_embedding(bits)` and forwards two batches (ragged multi-hot bags).  The fixture holds data only:
the initial parameters, the inputs, the fp32 predictions and the predictions with 4- and 8-bit tables.  tests/test_gpu_quant_emb.py loads
the parameters into this project's model on the device and must reproduce the predictions; tests/test_quant_emb_host.py checks them
against torch's operators on the CPU.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

M_SPA, LN_EMB, LN_BOT, B, STEPS, SEED = 16, [60, 3, 500, 1200], [13, 32, 16], 64, 2, 20
BITS = [4, 8]


def main() -> None:
    if not os.environ.get("DLRM_REFERENCE"):
        sys.exit("set DLRM_REFERENCE to a checkout of the reference (facebookresearch/dlrm)")
    import make_golden                                   # (reads DLRM_REFERENCE; stubs torch.utils.tensorboard)
    ref, _dp, _ext = make_golden.import_reference()
    F = len(LN_EMB) + 1
    ln_top = [M_SPA + F * (F - 1) // 2, 32, 1]

    def build():
        np.random.seed(SEED)
        return ref.DLRM_Net(M_SPA, np.asarray(LN_EMB), np.asarray(LN_BOT), np.asarray(ln_top), arch_interaction_op="dot",
                            sigmoid_top=len(ln_top) - 2, loss_function="bce")

    out = {}
    model = build()
    for k, v in model.state_dict().items():
        out["init." + k] = v.numpy().copy()
    rng = np.random.default_rng(SEED)
    batches = []
    for s in range(STEPS):
        X = rng.random((B, LN_BOT[0])).astype(np.float32)
        lS_o, lS_i = [], []
        for n in LN_EMB:
            lens = rng.integers(0, 5, size=B)
            lS_o.append(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
            lS_i.append(rng.integers(0, n, size=int(lens.sum())).astype(np.int64))
        batches.append((X, lS_o, lS_i))
        out[f"s{s}.X"] = X
        for k in range(len(LN_EMB)):
            out[f"s{s}.off{k}"], out[f"s{s}.idx{k}"] = lS_o[k], lS_i[k]
    for bits in [32] + BITS:
        m = build()
        m.quantize_embedding(bits)                       # (32: returns without change — the fp32 predictions)
        assert m.quantize_emb == (bits != 32)
        for s, (X, lS_o, lS_i) in enumerate(batches):
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):      # (the reference prints a debug line per table)
                Z = m(torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i])
            out[f"pred{bits}.s{s}"] = Z.numpy().copy()
    meta = {"m_spa": M_SPA, "ln_emb": LN_EMB, "ln_bot": LN_BOT, "ln_top": ln_top, "interaction": "dot", "sigmoid_top": len(ln_top) - 2,
            "batch": B, "steps": STEPS, "bits": BITS, "seed": SEED, "torch": torch.__version__}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "quant_inference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
