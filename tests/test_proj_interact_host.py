"""Host-side checks of torchrec_variant.DLRM_Projection (the projected interaction) — construction, initialisation order, refusals and bindings.
Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, D = [40, 9, 300], 16


def build(seed=2, branch1=(32, 32), branch2=(24, 48)):
    from dlrm_amd.torchrec_variant import DLRM_Projection
    np.random.seed(seed)
    return DLRM_Projection(ROWS, D, 13, [24, D], [32, 1], list(branch1), list(branch2))


def test_state_dict_keys_and_shapes():
    from dlrm_amd.torchrec_variant import DLRM
    model = build()
    assert (model.I1, model.I2) == (2, 3)
    assert model.top_l[0].in_features == 16 + 6
    assert model.proj1_l[0].in_features == model.proj2_l[0].in_features == 64
    np.random.seed(2)
    base = DLRM(ROWS, D, 13, [24, D], [32, 1])
    sd = model.state_dict()
    extra = {"proj1_l.0.weight": (32, 64), "proj1_l.0.bias": (32,), "proj1_l.2.weight": (32, 32), "proj1_l.2.bias": (32,),
             "proj2_l.0.weight": (24, 64), "proj2_l.0.bias": (24,), "proj2_l.2.weight": (48, 24), "proj2_l.2.bias": (48,)}
    assert set(sd) == set(base.state_dict()) | set(extra)
    assert list(sd)[-8:] == ["proj1_l.0.weight", "proj1_l.0.bias", "proj1_l.2.weight", "proj1_l.2.bias",
                             "proj2_l.0.weight", "proj2_l.0.bias", "proj2_l.2.weight", "proj2_l.2.bias"]
    for k, shape in extra.items():
        assert tuple(sd[k].shape) == shape, k
    for k, v in base.state_dict().items():
        want = (32, 22) if k == "top_l.0.weight" else tuple(v.shape)
        assert tuple(sd[k].shape) == want, k
    # every layer of a branch, the last included, is followed by a ReLU; the over arch ends with a bare Linear
    assert [type(m).__name__ for m in model.proj1_l] == ["Linear", "ReLU"] * 2 == [type(m).__name__ for m in model.proj2_l]
    assert [type(m).__name__ for m in model.top_l] == ["Linear", "ReLU", "Linear"]


def test_initialisation_is_a_function_of_the_numpy_seed():
    a, b, c = build(7).state_dict(), build(7).state_dict(), build(8).state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["proj2_l.2.weight"], c["proj2_l.2.weight"])
    # the tables and the two towers are drawn before the branches: a sibling built from the same seed starts with the same bits
    from dlrm_amd.torchrec_variant import DLRM
    np.random.seed(7)
    base = DLRM(ROWS, D, 13, [24, D], [32, 1]).state_dict()
    for k in base:
        if not k.startswith("top_l."):                      # (the top tower's input width differs)
            assert torch.equal(a[k], base[k]), k


def test_constructor_refuses_what_torchrec_refuses():
    from dlrm_amd.torchrec_variant import DLRM_Projection
    with pytest.raises(ValueError, match="multiple of the embedding dimension"):
        DLRM_Projection(ROWS, D, 13, [24, D], [32, 1], [32, 40], [24, 48])
    with pytest.raises(ValueError, match="multiple of the embedding dimension"):
        DLRM_Projection(ROWS, D, 13, [24, D], [32, 1], [32, 32], [24, 8])
    with pytest.raises(ValueError, match=re.escape("dense_arch_layer_sizes[-1] must equal the embedding dimension")):
        DLRM_Projection(ROWS, D, 13, [24, 8], [32, 1], [32, 32], [24, 48])


def test_quantisation_is_refused_like_the_siblings():
    from dlrm_amd import torchrec_variant as tv
    assert tv.DLRM_Projection.quantize_embedding is tv.DLRM_DCN.quantize_embedding
    assert tv.DLRM_Projection.quantize_mlp is tv.DLRM_DCN.quantize_mlp
    model = build()
    with pytest.raises(SystemExit, match=re.escape("ERROR: quantized embedding tables are built for DLRM_Net only, not for the torchrec variants "
                                                   "(DLRM_Projection)")):
        model.quantize_embedding(8)
    with pytest.raises(SystemExit, match=re.escape("ERROR: quantized MLP towers are built for DLRM_Net only, not for the torchrec variants "
                                                   "(DLRM_Projection)")):
        model.quantize_mlp(8)


def test_qr_md_and_bf16_tables_are_refused_like_the_siblings():
    import inspect
    from dlrm_amd import torchrec_variant as tv
    cls = tv.DLRM_Projection
    assert cls._qr_supported is False and cls._md_supported is False and cls._bf16_supported is False
    assert not any(p.startswith(("qr_", "md_")) or p == "kwargs" for p in inspect.signature(cls.__init__).parameters)
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.qr_flag, m.qr_threshold, m.qr_collisions, m.qr_operation = True, 200, 4, "mult"
    with pytest.raises(SystemExit, match="ERROR: QR embeddings are built for DLRM_Net only"):
        m.create_emb(8, np.asarray([300]))
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.md_flag, m.md_threshold = True, 2
    with pytest.raises(SystemExit, match="ERROR: mixed-dimension embeddings are built for DLRM_Net only"):
        m.create_emb([8, 4], np.asarray([300, 30]))
    with pytest.raises(SystemExit, match="ERROR: bfloat16 embedding tables are built for DLRM_Net only, not for the torchrec variants"):
        build().embedding_bfloat16()


def test_distributed_forward_is_refused(monkeypatch):
    from dlrm_amd import dlrm_net
    model = build()
    monkeypatch.setattr(dlrm_net.ext_dist, "is_distributed", lambda: True)
    with pytest.raises(SystemExit, match=re.escape("ERROR: DLRM_Projection is single-process only (the table-sharded distributed forward is "
                                                   "not built for it)")):
        model(torch.zeros((2, 13)), [torch.zeros(2, dtype=torch.int64)] * 3, [torch.zeros(2, dtype=torch.int64)] * 3)


def test_set_mlp_arith_reaches_the_branches():
    model = build()
    assert {t.arith for t in (model.bot_l, model.top_l, model.proj1_l, model.proj2_l)} == {"f32"}
    model.set_mlp_arith("bf16")
    assert [t.arith for t in (model.bot_l, model.top_l, model.proj1_l, model.proj2_l)] == ["bf16"] * 4
    with pytest.raises(Exception):
        model.set_mlp_arith("fp8")


def test_dlrm_train_wraps_it_unchanged():
    from dlrm_amd.torchrec_variant import DLRMTrain
    model = build()
    wrapped = DLRMTrain(model)
    assert wrapped.model is model
    assert set(wrapped.state_dict()) == {"model." + k for k in model.state_dict()}


def test_bindings_and_header_declare_both_symbols():
    from dlrm_amd import _lib, ops, functional
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    for name, nargs in (("dlrm_proj_interact_fwd", 13), ("dlrm_proj_interact_bwd", 17)):
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs
    assert "interact_proj.hip" in open(os.path.join(ROOT, "dlrm_amd", "csrc", "Makefile")).read()
    assert _lib.EXPECTED_ABI == 17          # symbols added, no signature changed
    assert callable(ops.proj_interact_fwd) and callable(ops.proj_interact_bwd) and hasattr(functional, "ProjectInteractFunction")
