"""Which launches DLRM_Net makes, and what it hands to the gradient sink, for every route of the fused lookup + interaction selection —
case by case against tests/fixtures/fused_route_trace.json.

The fixture holds, per case, the ordered list of launch categories (every `ops._timed` entered during one prediction or one training step)
and the list of sink calls (number of tables, shape of the gradient buffer, presorted or not) AS RECORDED FROM THE COMMIT BEFORE the selection
became one function (dlrm_net.fused_route) and the three gather Functions one: `python tests/test_gpu_fused_route.py --record FILE` in a
checkout of that commit with this file copied in.  It is never regenerated from newer code: a refactor of the selection must reproduce it.
tools/fused_route_identity.py runs the same cases for the bits."""
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "fused_route_trace.json")
FLAGS = ("fuse_emb_interact", "fuse_quant_interact", "fuse_qr_interact", "fuse_bf16_interact", "fuse_narrow_interact")
LN_EMB = {"fp32": [300, 24, 583, 150], "bf16": [300, 24, 583, 150], "quant": [300, 24, 583, 150],
          "qr": [460, 24, 383], "md": [460, 24, 383, 210, 90]}            # (QR / MD threshold 200)
NARROW = 32


def dev():
    return torch.device("cuda:0")


def cases():
    """(kind, D, bits, flag turned off | None, offsets state, B, "predict" | "step", extra | None).  Every route of the selection with all
    flags on (tagged offsets at B = 64 and 300, fresh at 300, ragged at 64, one prediction) and with each flag that admits it off; then the
    legs that hang off a route: the update inside the backward, the host-side proof, and the models no route takes."""
    out = []
    for kind, own in (("fp32", []), ("bf16", ["fuse_bf16_interact"]), ("qr", ["fuse_qr_interact"]), ("quant", ["fuse_quant_interact"])):
        run = "predict" if kind == "quant" else "step"
        for D in (128, NARROW):
            for bits in ((4, 8) if kind == "quant" else (0,)):
                out += [(kind, D, bits, None, "tagged", 64, run, None), (kind, D, bits, None, "tagged", 300, run, None),
                        (kind, D, bits, None, "fresh", 300, run, None), (kind, D, bits, None, "ragged", 64, run, None)]
                if run == "step":
                    out.append((kind, D, bits, None, "tagged", 64, "predict", None))
                    out.append((kind, D, bits, None, "fresh", 64, "predict", None))
                for off in ["fuse_emb_interact"] + own + (["fuse_narrow_interact"] if D != 128 else []):
                    out.append((kind, D, bits, off, "tagged", 64, run, None))
                    out.append((kind, D, bits, off, "fresh", 300, run, None))
            if kind == "quant":
                out.append((kind, D, 8, None, "tagged", 64, "step", None))           # a gradient is wanted through the bottom tower
    for state in ("tagged", "fresh", "ragged"):
        out.append(("fp32", 128, 0, None, state, 64, "step", "update_in_backward"))
        out.append(("fp32", 128, 0, None, state, 300, "step", "host_proof"))
        out.append(("fp32", 128, 0, None, state, 64, "predict", "host_proof"))
    out.append(("fp32", NARROW, 0, None, "tagged", 64, "step", "update_in_backward"))
    out.append(("bf16", 128, 0, None, "tagged", 64, "step", "update_in_backward"))
    out.append(("qr", 128, 0, None, "fresh", 64, "step", "host_proof"))
    out.append(("qr", NARROW, 0, None, "ragged", 64, "step", "host_proof"))
    out.append(("quant", 128, 8, None, "fresh", 64, "predict", "host_proof"))
    out.append(("md", 16, 0, None, "tagged", 64, "step", None))
    out.append(("md", 16, 0, None, "fresh", 300, "step", None))
    for kind, D in (("fp32", 128), ("fp32", NARROW), ("qr", 128), ("bf16", NARROW), ("quant", 128)):
        bits, run = (8, "predict") if kind == "quant" else (0, "step")
        out.append((kind, D, bits, None, "tagged", 64, run, "multihot"))
        out.append((kind, D, bits, None, "tagged", 64, run, "cat"))
    out.append(("fp32", 128, 0, None, "tagged", 64, "step", "pooling_weights"))
    out.append(("quant", NARROW, 4, None, "tagged", 64, "predict", "pooling_weights"))
    return out


def case_id(case):
    kind, D, bits, off, state, B, run, extra = case
    return "%s|D%d|bits%d|%s|%s|B%d|%s|%s" % (kind, D, bits, "all_on" if off is None else off + "=0", state, B, run, extra or "plain")


def build_model(kind, D, bits, off, extra):
    import dlrm_amd
    np.random.seed(7)
    torch.manual_seed(7)
    ln_emb = LN_EMB[kind]
    F = 1 + len(ln_emb)
    op = "cat" if extra == "cat" else "dot"
    n_top = D * F if op == "cat" else D + F * (F - 1) // 2
    kw = {}
    if kind == "qr":
        kw = dict(qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    if kind == "md":
        kw = dict(md_flag=True, md_threshold=200)
    if extra == "pooling_weights":
        kw["weighted_pooling"] = "fixed"
    m_spa = [16, 8, 4, 16, 2] if kind == "md" else D
    m = dlrm_amd.DLRM_Net(m_spa, np.asarray(ln_emb), np.asarray([13, 64, D]), np.asarray([n_top, 64, 1]), op, sigmoid_top=1,
                          loss_function="bce", **kw).to(dev())
    if kind == "bf16":
        m.embedding_bfloat16("stochastic", seed=3)
    for f in FLAGS:
        setattr(m, f, f != off)
    if extra == "update_in_backward":
        m.update_in_backward = True
    if kind == "quant":
        m.quantize_embedding(bits)
    return m


def make_batch(kind, B, state, extra, seed=11):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    hots = 3 if extra == "multihot" else 1
    X = torch.from_numpy(rng.random((B, 13)).astype(np.float32)).to(dev())
    lS_i = [torch.from_numpy(rng.integers(0, n, size=B * hots).astype(np.int64)).to(dev()) for n in LN_EMB[kind]]
    target = torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32)).to(dev())
    lS_o = [torch.arange(B, device=dev()) * hots for _ in LN_EMB[kind]]
    if state == "tagged":
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    if state == "ragged":
        lS_o[1][17] = 16                   # bag 16 has two lookups, bag 17 none: nnz == B, not one lookup per bag
    return X, lS_o, lS_i, target


def run_case(case, mp):
    """-> (launch categories in order, sink calls, {name: tensor} of the prediction, the loss and every parameter after the step)"""
    from dlrm_amd import dlrm_net as _net, ops
    from dlrm_amd.optim import FusedSGD
    kind, D, bits, off, state, B, run, extra = case
    model = build_model(kind, D, bits, off, extra)
    steps = 2 if extra == "update_in_backward" else 1              # (the first step binds the optimizer, the second updates in backward)
    batches = [make_batch(kind, B, state, extra, seed=11 + s) for s in range(steps)]
    torch.cuda.synchronize()
    launches, sinks = [], []

    class Recorded(ops._timed):
        def __enter__(self):
            launches.append(self.name)
            return super().__enter__()

    stash = _net.DLRM_Net._stash_embedding_grad

    def recorded_stash(self, weights, bags, dout, presorted=None):
        sinks.append([len(weights), list(dout.shape), presorted is not None])
        return stash(self, weights, bags, dout, presorted)

    mp.setattr(ops, "_timed", Recorded)
    mp.setattr(_net.DLRM_Net, "_stash_embedding_grad", recorded_stash)
    if extra == "host_proof":
        mp.setattr(_net, "DEVICE_PREDICATE", False)
    out = {}
    if run == "predict":
        X, lS_o, lS_i, _ = batches[0]
        with torch.no_grad():
            out["Z"] = model(X, lS_o, lS_i)
    else:
        opt = (FusedSGD if extra == "update_in_backward" else torch.optim.SGD)(model.parameters(), lr=0.1)
        for s, (X, lS_o, lS_i, target) in enumerate(batches):
            launches.append("-- step %d" % s)
            opt.zero_grad()
            Z = model(X, lS_o, lS_i)
            loss = model.loss_fn(Z, target)
            launches.append("-- backward")
            loss.backward()
            launches.append("-- optimizer")
            opt.step()
            out["Z%d" % s], out["loss%d" % s] = Z.detach(), loss.detach()
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    for k, v in model.state_dict().items():
        out[k] = v
    for k, q in enumerate(model.emb_l_q or []):
        out["emb_l_q.%d" % k] = q
    return launches, sinks, out


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_launches_and_sink_calls_equal_the_recorded_ones(case, monkeypatch):
    want = json.load(open(FIXTURE))[case_id(case)]
    launches, sinks, _ = run_case(case, monkeypatch)
    assert {"launches": launches, "sinks": sinks} == want


if __name__ == "__main__":
    # python tests/test_gpu_fused_route.py --record FILE: write the fixture from the dlrm_amd package of THIS checkout.  Every case runs twice,
    # the second time in reverse order: a trace that depended on what ran before it would not be a fixture.
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True)
    args = ap.parse_args()
    t0 = time.perf_counter()
    passes = []
    for order in (cases(), cases()[::-1]):
        got = {}
        for case in order:
            with pytest.MonkeyPatch.context() as mp:
                launches, sinks, _ = run_case(case, mp)
            got[case_id(case)] = {"launches": launches, "sinks": sinks}
        passes.append(got)
    assert passes[0] == passes[1], sorted(k for k in passes[0] if passes[0][k] != passes[1][k])
    assert len(passes[0]) == len(cases())
    with open(args.record, "w") as f:
        json.dump(passes[0], f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases twice in %.1f s" % (len(cases()), time.perf_counter() - t0))
