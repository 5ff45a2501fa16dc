"""Quantised embedding tables, host side: the oracles the GPU tests (tests/test_gpu_quant_emb.py) use are pinned here against torch's own
CPU operators, and the model surface is checked as far as it goes without a device.

  * np_pack8 / np_pack4: a numpy restatement of torch's fused row-wise formats (`embedding_bag_byte_prepack`, `embedding_bag_4bit_prepack`),
    required to equal them BYTE FOR BYTE;
  * dequant_sum_f64: sum_i p_i (s_r q + b_r) of packed rows in float64, with the magnitude sum_i |p_i| (|s_r| q + |b_r|) the error bound
    is stated in:   |err| <= (L + 2) * 2^-23 * magnitude   (L = bag length: at most 2 roundings per dequantised term, L - 1 for the in-order
    sum; derived, not measured);
  * torch_quant_forward: the reference's quantised forward composed from torch's operators (prepack + *_rowwise_offsets per table, plain
    torch for the towers and the dot / cat interaction);
  * tests/golden/quant_inference.npz (tools/make_golden_quant.py: the live reference's predictions) is checked against that composition,
    so a stale fixture cannot pass silently.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

PRED_RTOL, PRED_ATOL = 2e-5, 1e-6            # the project's prediction tolerance (smoke(), tests/test_gpu_model.py)
EPS23 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ pack oracles
def np_pack8(W: np.ndarray) -> np.ndarray:
    W = np.ascontiguousarray(W, dtype=np.float32)
    rows, D = W.shape
    mn, mx = W.min(axis=1), W.max(axis=1)
    rng_ = (mx - mn).astype(np.float32)
    scale = (rng_ / np.float32(255.0)).astype(np.float32)
    inv = (np.float32(255.0) / (rng_ + np.float32(1e-8)).astype(np.float32)).astype(np.float32)
    q = np.rint(((W - mn[:, None]).astype(np.float32) * inv[:, None]).astype(np.float32))
    q = np.clip(q, 0, 255).astype(np.uint8)
    out = np.empty((rows, D + 8), dtype=np.uint8)
    out[:, :D] = q
    out[:, D:D + 4] = scale.view(np.uint8).reshape(rows, 4)
    out[:, D + 4:] = mn.astype(np.float32).view(np.uint8).reshape(rows, 4)
    return out


def np_pack4(W: np.ndarray) -> np.ndarray:
    W = np.ascontiguousarray(W, dtype=np.float32)
    rows, D = W.shape
    assert D % 2 == 0
    with np.errstate(divide="ignore", over="ignore"):
        mn16 = W.min(axis=1).astype(np.float16)
        mn = mn16.astype(np.float32)
        rng_ = (W.max(axis=1) - mn).astype(np.float32)
        scale16 = np.where(rng_ == 0, np.float32(1.0), (rng_ / np.float32(15.0)).astype(np.float32)).astype(np.float32).astype(np.float16)
        scale = scale16.astype(np.float32)
        scale = np.where(scale == 0, np.float32(1.0), scale).astype(np.float32)
        inv = (np.float32(1.0) / scale).astype(np.float32)
        bad = np.isinf(inv)
        scale = np.where(bad, np.float32(1.0), scale).astype(np.float32)
        inv = np.where(bad, np.float32(1.0), inv).astype(np.float32)
    q = np.rint(((W - mn[:, None]).astype(np.float32) * inv[:, None]).astype(np.float32))
    q = np.clip(q, 0, 15).astype(np.uint8)
    out = np.empty((rows, D // 2 + 4), dtype=np.uint8)
    out[:, :D // 2] = q[:, 0::2] | (q[:, 1::2] << 4)
    out[:, D // 2:D // 2 + 2] = scale.astype(np.float16).view(np.uint8).reshape(rows, 2)
    out[:, D // 2 + 2:] = mn16.view(np.uint8).reshape(rows, 2)
    return out


def np_pack(W, bits):
    return np_pack8(W) if bits == 8 else np_pack4(W)


def torch_pack(W: np.ndarray, bits: int) -> np.ndarray:
    op = torch.ops.quantized.embedding_bag_byte_prepack if bits == 8 else torch.ops.quantized.embedding_bag_4bit_prepack
    return op(torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32))).numpy()


def unpack(packed: np.ndarray, bits: int, D: int):
    """(q [rows, D] float64, scale [rows] float64, bias [rows] float64) of packed rows"""
    packed = np.ascontiguousarray(packed)
    rows = packed.shape[0]
    if bits == 8:
        q = packed[:, :D].astype(np.float64)
        sb = packed[:, D:D + 8].copy().view(np.float32).reshape(rows, 2).astype(np.float64)
    else:
        b = packed[:, :D // 2]
        q = np.empty((rows, D), dtype=np.float64)
        q[:, 0::2] = b & 15
        q[:, 1::2] = b >> 4
        sb = packed[:, D // 2:D // 2 + 4].copy().view(np.float16).reshape(rows, 2).astype(np.float64)
    return q, sb[:, 0], sb[:, 1]


def special_weights(rows: int, D: int, seed: int) -> np.ndarray:
    """rows of the reference's init (uniform(+-sqrt(1/n))) with, where the table is long enough, constant rows, all-zero rows and rows
    scaled by 1e4 and 1e-6 mixed in"""
    rng = np.random.default_rng(seed)
    bound = np.sqrt(1.0 / rows)
    W = rng.uniform(-bound, bound, size=(rows, D)).astype(np.float32)
    if rows >= 8:
        W[1] = 0.0
        W[2] = 0.37
        W[3] = -1.25e-3
        W[4] *= np.float32(1e4)
        W[5] *= np.float32(1e-6)
        W[6] = np.abs(W[6])
        W[7, 1:] = W[7, 0]
    if rows >= 64:
        k = rows // 8
        W[k:2 * k] *= np.float32(1e4)
        W[2 * k:3 * k] *= np.float32(1e-6)
        W[3 * k:3 * k + 8] = 0.0
        W[3 * k + 8:3 * k + 16] = rng.standard_normal((8, 1)).astype(np.float32)
    return W


def ragged_bags(rng, rows: int, B: int, max_len: int, weighted: bool):
    lens = rng.integers(0, max_len + 1, size=B)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx = rng.integers(0, rows, size=int(lens.sum())).astype(np.int64)
    psw = rng.uniform(-2.0, 2.0, size=idx.size).astype(np.float32) if weighted else None
    return off, idx, psw


# ------------------------------------------------------------------------------------------------ lookup oracle
def dequant_sum_f64(packed: np.ndarray, bits: int, D: int, idx: np.ndarray, off: np.ndarray, psw=None, skip_out_of_range=False):
    """(value [B, D], magnitude [B, D], L [B]) in float64 for bags [off[b], off[b+1]) with off[B] := len(idx)"""
    idx = np.asarray(idx, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    B = off.size
    p = np.ones(idx.size) if psw is None else np.asarray(psw, dtype=np.float64)
    ok = (idx >= 0) & (idx < packed.shape[0])
    assert skip_out_of_range or ok.all()
    safe = np.where(ok, idx, 0)
    q, s, b = unpack(packed[safe], bits, D)
    p = np.where(ok, p, 0.0)
    term = p[:, None] * (s[:, None] * q + b[:, None])
    mag = np.abs(p)[:, None] * (np.abs(s)[:, None] * q + np.abs(b)[:, None])
    ends = np.concatenate([off[1:], [idx.size]])
    L = ends - off
    bag = np.repeat(np.arange(B), L)
    val = np.zeros((B, D))
    m = np.zeros((B, D))
    np.add.at(val, bag, term)
    np.add.at(m, bag, mag)
    return val, m, L


def assert_within_bound(got: np.ndarray, val: np.ndarray, mag: np.ndarray, L: np.ndarray, factor: float = 1.0, what: str = ""):
    bound = factor * (L[:, None] + 2) * EPS23 * mag
    err = np.abs(got.astype(np.float64) - val)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: worst |err| / bound = %.3f (factor %g)" % (what, worst, factor))
    assert (err <= bound).all(), "%s: |err| exceeds %g * (L + 2) * 2^-23 * sum |p|(|s| q + |b|): worst ratio %.3f" % (what, factor, worst)


def torch_lookup(packed: np.ndarray, bits: int, idx, off, psw=None) -> np.ndarray:
    op = (torch.ops.quantized.embedding_bag_byte_rowwise_offsets if bits == 8 else torch.ops.quantized.embedding_bag_4bit_rowwise_offsets)
    w = None if psw is None else torch.from_numpy(np.asarray(psw, dtype=np.float32))
    return op(torch.from_numpy(np.ascontiguousarray(packed)), torch.from_numpy(np.asarray(idx, dtype=np.int64)),
              torch.from_numpy(np.asarray(off, dtype=np.int64)), per_sample_weights=w).numpy()


# ------------------------------------------------------------------------------------------------ model composition
def torch_quant_forward(params: dict, bits: int, X, lS_o, lS_i, interaction="dot", itself=False, sigmoid_bot=-1, sigmoid_top=-1,
                        pool_w=None) -> np.ndarray:
    """the reference's quantised forward (dlrm_s_pytorch.py:430-450, 483-510, 587-612) from torch's CPU operators.  params: a state_dict
    as numpy arrays (`emb_l.{k}.weight`, `bot_l.{2i}.weight|bias`, `top_l.{2i}...`); pool_w: per-table row weights (fixed pooling)."""
    def tower(x, prefix, sig):
        i = 0
        while f"{prefix}.{2 * i}.weight" in params:
            W, b = torch.from_numpy(params[f"{prefix}.{2 * i}.weight"]), torch.from_numpy(params[f"{prefix}.{2 * i}.bias"])
            x = torch.nn.functional.linear(x, W, b)
            x = torch.sigmoid(x) if i == sig else torch.relu(x)
            i += 1
        return x

    with torch.no_grad():
        x = tower(torch.from_numpy(np.asarray(X, dtype=np.float32)), "bot_l", sigmoid_bot)
        ly = []
        for k in range(len(lS_i)):
            packed = torch_pack(params[f"emb_l.{k}.weight"], bits)
            idx = np.asarray(lS_i[k], dtype=np.int64)
            psw = None if pool_w is None else np.asarray(pool_w[k], dtype=np.float32)[idx]
            ly.append(torch.from_numpy(torch_lookup(packed, bits, idx, lS_o[k], psw)))
        if interaction == "dot":
            B, d = x.shape
            T = torch.cat([x] + ly, dim=1).view((B, -1, d))
            Z = torch.bmm(T, torch.transpose(T, 1, 2))
            ni = T.shape[1]
            off = 1 if itself else 0
            li = torch.tensor([i for i in range(ni) for j in range(i + off)])
            lj = torch.tensor([j for i in range(ni) for j in range(i + off)])
            R = torch.cat([x, Z[:, li, lj]], dim=1)
        else:
            R = torch.cat([x] + ly, dim=1)
        return tower(R, "top_l", sigmoid_top).numpy()


# ------------------------------------------------------------------------------------------------ tests
PACK_SHAPES = [(300, 8), (1000, 16), (4000, 32), (2000, 64), (1500, 128), (700, 256)]


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("rows,D", PACK_SHAPES)
def test_numpy_pack_equals_torch_prepack_byte_for_byte(bits, rows, D):
    W = special_weights(rows, D, seed=rows + D + bits)
    assert np.array_equal(np_pack(W, bits), torch_pack(W, bits))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("weighted", [False, True])
def test_fp64_lookup_oracle_against_torch_rowwise_offsets(bits, weighted):
    rng = np.random.default_rng(7 + bits)
    rows, D, B = 3000, 64, 512
    packed = np_pack(special_weights(rows, D, seed=11), bits)
    off, idx, psw = ragged_bags(rng, rows, B, 39, weighted)
    val, mag, L = dequant_sum_f64(packed, bits, D, idx, off, psw)
    assert_within_bound(torch_lookup(packed, bits, idx, off, psw), val, mag, L, what="torch CPU %d-bit" % bits)


def _tiny_model():
    import dlrm_amd
    np.random.seed(3)
    ln_emb = np.asarray([40, 3, 200])
    return dlrm_amd.DLRM_Net(16, ln_emb, np.asarray([13, 32, 16]), np.asarray([16 + 6, 32, 1]), "dot", sigmoid_top=1, loss_function="bce")


def test_quantize_embedding_on_a_cpu_model_names_the_gpu():
    model = _tiny_model()
    with pytest.raises(RuntimeError, match="GPU") as e:
        model.quantize_embedding(8)
    assert "CPU-only" not in str(e.value) and "device first" in str(e.value)
    assert model.quantize_emb is False and model.emb_l is not None and model.quantize_bits == 32 and model.emb_l_q == []


def test_quantize_embedding_with_other_bits_is_a_no_op():
    model = _tiny_model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert model.quantize_embedding(32) is None
    assert model.quantize_emb is False and model.quantize_bits == 32 and model.emb_l_q == [] and len(model.emb_l) == 3
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_operators_need_a_gpu():
    from dlrm_amd import ops
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.emb_quantize(torch.zeros(4, 8), 8)
    assert ops.quant_row_bytes(128, 8) == 136 and ops.quant_row_bytes(128, 4) == 68
    with pytest.raises(RuntimeError):
        ops.quant_row_bytes(7, 4)


def test_torchrec_variants_refuse_quantisation():
    from dlrm_amd import torchrec_variant as tv
    np.random.seed(5)
    m = tv.DLRM([30, 5], 8, 13, [16, 8], [16, 1])
    with pytest.raises(SystemExit, match="ERROR: quantized embedding tables are built for DLRM_Net only"):
        m.quantize_embedding(8)
    assert tv.ShardedDLRM.quantize_embedding is tv.DLRM.quantize_embedding is tv.DLRM_DCN.quantize_embedding


def test_fixture_predictions_equal_the_torch_operator_composition():
    d, meta = load_golden("quant_inference")
    params = {k[len("init."):]: v for k, v in d.items() if k.startswith("init.")}
    T = len(meta["ln_emb"])
    for bits in meta["bits"]:
        for s in range(meta["steps"]):
            want = d[f"pred{bits}.s{s}"]
            got = torch_quant_forward(params, bits, d[f"s{s}.X"], [d[f"s{s}.off{k}"] for k in range(T)], [d[f"s{s}.idx{k}"] for k in range(T)],
                                      interaction=meta["interaction"], sigmoid_top=meta["sigmoid_top"])
            np.testing.assert_allclose(got, want, rtol=PRED_RTOL, atol=PRED_ATOL, err_msg="bits %d step %d" % (bits, s))
        # the quantised predictions must differ from the fp32 ones, or the fixture would not see the tables at all
        assert not np.allclose(d[f"pred{bits}.s0"], d["pred32.s0"], rtol=1e-7, atol=0)
