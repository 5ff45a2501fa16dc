"""Which launches the two-kernel embedding path and the sparse update behind it make, and with which arguments, for every table kind, optimizer
and model switch — case by case against tests/fixtures/emb_update_trace.json.

The fixture holds, per case: the ordered list of launch categories (every `ops._timed` entered during two training steps, with `-- step` /
`-- backward` / `-- optimizer` markers between them); every call of a C symbol that begins dlrm_emb_fwd, dlrm_emb_bwd_ or dlrm_emb_presort —
the symbol and its arguments in ABI order: numbers by value, pointers as "null" / "ptr", pointers to a table or to an optimizer state tensor
by name ("W2", "state[2].momentum"), arrays element by element, the stream as "main" / "side" —; and the message of the SystemExit or
RuntimeError the case ends in, if it does.  It was RECORDED FROM THE COMMIT BEFORE the update wrappers of ops.py became one body over
ops.UPDATE_KINDS and DLRM_Net's three answers to "which kernel updates these tables" one executor: `python tests/test_gpu_emb_update.py --record
FILE` in a checkout of that commit with this file copied in.  It is never regenerated from newer code: a refactor of this path must reproduce
it.  tools/emb_update_identity.py runs the same cases for the bits."""
import ctypes as C
import gc
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

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "emb_update_trace.json")
RECORDED = ("dlrm_emb_fwd", "dlrm_emb_bwd_", "dlrm_emb_presort")
LN_EMB = {"plain": [300, 24, 583, 150], "qr": [460, 24, 383], "md": [460, 24, 383, 210, 90]}            # (QR / MD threshold 200)
B = 64
# table kind -> (LN_EMB key, D, bfloat16 rounding | None, pooling weights | None)
TABLES = {"fp32_16": ("plain", 16, None, None), "fp32_128": ("plain", 128, None, None), "bf16_stochastic": ("plain", 16, "stochastic", None),
          "bf16_nearest": ("plain", 128, "nearest", None), "qr": ("qr", 16, None, None), "md": ("md", 16, None, None),
          "fp32_fixed": ("plain", 16, None, "fixed"), "bf16_fixed": ("plain", 16, "stochastic", "fixed"), "fp32_learned": ("plain", 16, None, "learned")}
OPTIMIZERS = ("sgd", "fused_sgd", "sgd_momentum", "rwsadagrad", "fused_adagrad", "adagrad", "adagrad_fused_on", "adam")


def dev():
    return torch.device("cuda:0")


def cases():
    """(tables, optimizer, model switch | None, batch, loop).  batch: "multihot" (3 lookups per bag: duplicate rows, nnz != B — the two-kernel
    lookup), "onehot" (untagged offsets: the lookup behind the launch predicate) or "tagged" (proven one lookup per bag).  loop: "steps" (two
    training steps), "accumulate" (two backward passes before one step), "owner_last" (an optimizer that holds only the dense parameters
    steps first, then the tables' owner) or "lr" (apply_pending_embedding_updates(lr=...), no optimizer).  Every (tables, optimizer) pair
    with defaults — the seven refusals among them —, then the switches and loops on the pairs they bear on."""
    out = [(t, o, None, "multihot", "steps") for t in TABLES for o in OPTIMIZERS
           if TABLES[t][3] is None or o in ("sgd", "rwsadagrad", "fused_adagrad", "adam")]          # (pooling weights do not choose the update)
    out += [(t, "sgd", None, "onehot", "steps") for t in TABLES]
    for t in ("fp32_128", "bf16_stochastic", "qr", "md", "fp32_learned"):
        out += [(t, o, "overlap_streams", "multihot", "steps") for o in ("sgd", "rwsadagrad")]
    out += [("fp32_128", "sgd", "overlap_streams", "onehot", "steps"), ("fp32_128", "fused_adagrad", "overlap_streams", "multihot", "steps"),
            ("fp32_16", "adam", "overlap_streams", "multihot", "steps")]
    out += [("fp32_128", "fused_sgd", "update_in_backward", b, "steps") for b in ("tagged", "onehot", "multihot")]
    out += [("fp32_128", "fused_sgd", "update_in_backward+overlap_streams", "tagged", "steps"),
            ("fp32_128", "fused_sgd", "update_in_backward", "tagged", "owner_last"), ("bf16_nearest", "fused_sgd", "update_in_backward", "tagged", "steps")]
    out += [(t, o, "fused_emb_update=0", "multihot", "steps") for t, o in (("fp32_16", "sgd"), ("fp32_16", "adam"), ("fp32_16", "adagrad"),
            ("fp32_learned", "sgd_momentum"), ("qr", "sgd"), ("md", "adagrad"), ("bf16_stochastic", "sgd"), ("bf16_nearest", "rwsadagrad"))]
    out += [(t, "sgd", "upd_atomic", "multihot", "steps") for t in ("fp32_16", "fp32_128", "qr", "md", "bf16_stochastic")]
    out += [(t, None, s, "multihot", "lr") for t in ("fp32_128", "bf16_stochastic", "bf16_nearest", "qr") for s in (None, "overlap_streams")]
    out += [(t, o, None, "multihot", "accumulate") for t in ("fp32_16", "bf16_stochastic", "qr") for o in ("sgd", "rwsadagrad", "fused_adagrad")]
    out += [("fp32_16", "adagrad_fused_on", None, "multihot", "accumulate"), ("fp32_16", "sgd_momentum", None, "multihot", "accumulate"),
            ("fp32_128", "sgd", "overlap_streams", "multihot", "accumulate")]
    out += [(t, o, s, "multihot", "owner_last") for t in ("fp32_16", "bf16_stochastic", "md") for o in ("sgd", "rwsadagrad") for s in (None, "overlap_streams")]
    return out


def case_id(case):
    tables, opt, switch, batch, loop = case
    return "%s|%s|%s|%s|%s" % (tables, opt or "no_optimizer", switch or "defaults", batch, loop)


def build_model(tables, opt, switch):
    import dlrm_amd
    from dlrm_amd import ops
    np.random.seed(7)
    torch.manual_seed(7)
    rows, D, rounding, pooling = TABLES[tables]
    ln_emb = LN_EMB[rows]
    F = 1 + len(ln_emb)
    kw = {}
    if rows == "qr":
        kw = dict(qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    if rows == "md":
        kw = dict(md_flag=True, md_threshold=200)
    if pooling is not None:
        kw["weighted_pooling"] = pooling
    m_spa = [16, 8, 4, 16, 2] if rows == "md" else D
    m = dlrm_amd.DLRM_Net(m_spa, np.asarray(ln_emb), np.asarray([13, 64, D]), np.asarray([D + F * (F - 1) // 2, 64, 1]), "dot", sigmoid_top=1,
                          loss_function="bce", **kw).to(dev())
    if rounding is not None:
        m.embedding_bfloat16(rounding, seed=3)
    for s in (switch or "").split("+"):
        if s in ("overlap_streams", "update_in_backward"):
            setattr(m, s, True)
        elif s == "fused_emb_update=0":
            m.fused_emb_update = False
        elif s == "upd_atomic":
            m.emb_update_mode = ops.UPD_ATOMIC
    m.fused_adagrad = opt == "adagrad_fused_on"
    return m


def build_optimizer(name, params):
    from dlrm_amd.optim import FusedAdagrad, FusedRWSAdagrad, FusedSGD
    params = list(params)
    if name == "sgd":
        return torch.optim.SGD(params, lr=0.1)
    if name == "fused_sgd":
        return FusedSGD(params, lr=0.1)
    if name == "sgd_momentum":
        return torch.optim.SGD(params, lr=0.1, momentum=0.9)
    if name == "rwsadagrad":
        return FusedRWSAdagrad(params, lr=0.05, lr_decay=0.01, eps=1e-8)
    if name == "fused_adagrad":
        return FusedAdagrad(params, lr=0.05, lr_decay=0.01, eps=1e-8)
    if name in ("adagrad", "adagrad_fused_on"):
        return torch.optim.Adagrad(params, lr=0.05, lr_decay=0.01, eps=1e-8)
    if name == "adam":
        return torch.optim.Adam(params, lr=0.01)
    raise ValueError(name)


def make_batch(tables, batch, seed):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    ln_emb = LN_EMB[TABLES[tables][0]]
    hots = 3 if batch == "multihot" else 1
    X = torch.from_numpy(rng.random((B, 13)).astype(np.float32)).to(dev())
    lS_i = [torch.from_numpy(rng.integers(0, n, size=B * hots).astype(np.int64)).to(dev()) for n in ln_emb]
    target = torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32)).to(dev())
    lS_o = [torch.arange(B, device=dev()) * hots for _ in ln_emb]
    if batch == "tagged":
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    return X, lS_o, lS_i, target


class RecordingLib:
    """stands where _lib.load() stands: every call of a RECORDED symbol is described and appended to `calls`, then made"""

    def __init__(self, lib, calls, model, optimizers):
        self._lib, self._calls, self._model, self._optimizers = lib, calls, model, optimizers

    def _names(self):
        """device address -> name, of the tables (index in model._emb_weights) and of their optimizer state tensors, as they are NOW"""
        names = {}
        for k, w in enumerate(self._model._emb_weights(self._model.emb_l)):
            names[w.data_ptr()] = "W%d" % k
            for opt in self._optimizers:
                for key, t in opt.state.get(w, {}).items():
                    if isinstance(t, torch.Tensor) and t.is_cuda and t.layout == torch.strided:      # (SGD's momentum of a COO gradient is sparse)
                        names[t.data_ptr()] = "state[%d].%s" % (k, key)
        return names

    def _describe(self, a, names):
        if a is None:
            return "null"
        if isinstance(a, (int, float)):
            return a
        if isinstance(a, C.c_void_p):
            return names.get(a.value, "ptr") if a.value else "null"
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return [names.get(v, "ptr") if v else "null" for v in a]
            return [int(v) for v in a]
        raise TypeError("argument %r of a recorded call" % (a,))

    def __getattr__(self, symbol):
        fn = getattr(self._lib, symbol)
        if not symbol.startswith(RECORDED):
            return fn

        def call(*args):
            from dlrm_amd.functional import _side_stream
            names = self._names()
            described = [self._describe(a, names) for a in args]
            if isinstance(args[-1], C.c_void_p):                        # (the workspace-size queries take no stream)
                st = args[-1].value or 0
                assert st in (_side_stream(dev()).cuda_stream, torch.cuda.default_stream(dev()).cuda_stream), (symbol, st)
                described[-1] = "side" if st == _side_stream(dev()).cuda_stream else "main"
            self._calls.append([symbol] + described)
            return fn(*args)
        return call


def run_case(case, mp):
    """-> ({"launches", "calls", "error"}, {name: tensor} of the losses, every parameter and every optimizer state tensor after the loop)"""
    from dlrm_amd import _lib, ops
    from dlrm_amd import dlrm_net as _net
    tables, opt_name, switch, batch, loop = case
    launches, calls, tensors = [], [], {}
    error = None

    class Recorded(ops._timed):
        def __enter__(self):
            launches.append(self.name)
            return super().__enter__()

    mp.setattr(ops, "_timed", Recorded)
    mp.setattr(ops, "_scratch_ws", {})                 # (the cached workspace only grows: its size must not depend on the cases before this one)
    model = build_model(tables, opt_name, switch)
    emb = {id(w) for w in model._emb_weights(model.emb_l)}
    if loop == "owner_last":
        optimizers = [build_optimizer(opt_name, (p for p in model.parameters() if id(p) not in emb)),
                      build_optimizer(opt_name, (p for p in model.parameters() if id(p) in emb))]
    else:
        optimizers = [build_optimizer(opt_name, model.parameters())] if opt_name is not None else []
    mp.setattr(_lib, "load", lambda lib=RecordingLib(_lib.load(), calls, model, optimizers): lib)
    batches = [make_batch(tables, batch, seed=11 + s) for s in range(2)]
    torch.cuda.synchronize()
    try:
        for s, (X, lS_o, lS_i, target) in enumerate(batches):
            launches.append("-- step %d" % s)
            if loop != "accumulate" or s == 0:
                for opt in optimizers:
                    opt.zero_grad()
            Z = model(X, lS_o, lS_i)
            loss = model.loss_fn(Z, target)
            launches.append("-- backward")
            loss.backward()
            tensors["loss%d" % s] = loss.detach()
            if loop == "accumulate" and s == 0:
                continue
            launches.append("-- optimizer")
            if loop == "lr":
                model.apply_pending_embedding_updates(lr=0.05)
                model._join_side_stream()
            for k, opt in enumerate(optimizers):
                if k:
                    launches.append("-- optimizer (the tables' owner); parked: %d" % len(model._pending_emb))
                opt.step()
    except (SystemExit, RuntimeError) as e:
        error = "%s: %s" % (type(e).__name__, e)
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    model._join_side_stream()
    model._pending_emb.clear()                         # (a case that ended in a refusal leaves its gradient parked)
    for k, v in model.state_dict().items():
        tensors[k] = v
    for n, opt in enumerate(optimizers):
        for k, p in enumerate(q for g in opt.param_groups for q in g["params"]):
            for key, t in sorted(opt.state.get(p, {}).items()):
                if isinstance(t, torch.Tensor):
                    tensors["optimizer%d.state[%d].%s" % (n, k, key)] = t
    del model, optimizers
    gc.collect()
    return {"launches": launches, "calls": calls, "error": error}, tensors


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_launches_and_c_calls_equal_the_recorded_ones(case, recorded, monkeypatch):
    got, _ = run_case(case, monkeypatch)
    assert json.loads(json.dumps(got)) == recorded[case_id(case)]


if __name__ == "__main__":
    # python tests/test_gpu_emb_update.py --record FILE: write the fixture from the dlrm_amd package of THIS checkout.  Every case runs twice,
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
                got[case_id(case)] = json.loads(json.dumps(run_case(case, mp)[0]))
        passes.append(got)
    assert passes[0] == passes[1], sorted(k for k in passes[0] if passes[0][k] != passes[1][k])
    assert len(passes[0]) == len(cases())
    with open(args.record, "w") as f:                  # (one line per case)
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(passes[0].items())) + "\n}\n")
    print("%d cases twice in %.1f s; %d end in an error" % (len(cases()), time.perf_counter() - t0, sum(1 for v in passes[0].values() if v["error"])))
