"""Quantised embedding tables on the device: dlrm_emb_quantize_rows / dlrm_emb_fwd_quant through dlrm_amd.ops, and
DLRM_Net.quantize_embedding + forward / evaluate.inference.

  * prepack: BYTE FOR BYTE `torch.ops.quantized.embedding_bag_{byte,4bit}_prepack` of the same weights on the CPU;
  * lookup: within (L + 2) * 2^-23 * sum_i |p_i| (|s_r| q + |b_r|) of the float64 evaluation of the packed bytes (derived in
    tests/test_quant_emb_host.py, whose oracles are pinned against torch there), and within twice that of torch's CPU operator;
  * model: predictions against the reference's quantised forward composed from torch's operators, and against the live reference's
    predictions (tests/golden/quant_inference.npz), at the project's prediction tolerance rtol 2e-5 / atol 1e-6.
"""
import numpy as np
import pytest
import torch

import test_quant_emb_host as H
from conftest import load_golden, params_with_prefix

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ prepack
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", [8, 12, 16, 64, 128, 256])
@pytest.mark.parametrize("rows", [1, 3, 2000, 100003])
def test_prepack_equals_torch_byte_for_byte(bits, D, rows):
    from dlrm_amd import ops
    W = H.special_weights(rows, D, seed=rows * 7 + D + bits)
    got = ops.emb_quantize(to_dev(W), bits)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (rows, ops.quant_row_bytes(D, bits))
    want = H.torch_pack(W, bits)
    got = got.cpu().numpy()
    diff = int((got != want).sum())
    assert diff == 0, "%d differing bytes in %d rows" % (diff, int((got != want).any(axis=1).sum()))


@pytest.mark.parametrize("bits", [8, 4])
def test_prepack_of_the_reference_init_equals_torch(bits):
    import dlrm_amd
    from dlrm_amd import ops
    np.random.seed(17)
    model = dlrm_amd.DLRM_Net(64, np.asarray([5000, 3, 77]), np.asarray([13, 64]), np.asarray([64 + 6, 1]), "dot")
    for e in model.emb_l:
        W = e.weight.detach()
        assert np.array_equal(ops.emb_quantize(W.to(dev()), bits).cpu().numpy(), H.torch_pack(W.numpy(), bits))


def test_prepack_of_an_unaligned_table_takes_the_plain_path():
    from dlrm_amd import ops
    W = H.special_weights(501, 16, seed=3)
    buf = torch.empty(501 * 16 + 1, device=dev())
    view = buf[1:].view(501, 16)                       # 4-byte aligned only
    view.copy_(to_dev(W))
    for bits in (8, 4):
        assert np.array_equal(ops.emb_quantize(view, bits).cpu().numpy(), H.torch_pack(W, bits))


# ------------------------------------------------------------------------------------------------ lookup
def make_tables(rows_list, D, bits, seed):
    """packed device tables + their bytes on the host.  Small tables come from special_weights (and so are also checked against torch's
    prepack); tables above 200k rows are drawn on the device."""
    from dlrm_amd import ops
    q_dev, q_host = [], []
    for t, n in enumerate(rows_list):
        if n <= 200000:
            W = to_dev(H.special_weights(n, D, seed=seed + t))
        else:
            g = torch.Generator(device=dev()).manual_seed(seed + t)
            W = (torch.rand((n, D), device=dev(), generator=g) - 0.5) * (2.0 / np.sqrt(n))
        q = ops.emb_quantize(W, bits)
        del W
        q_dev.append(q)
        q_host.append(q.cpu().numpy())
    return q_dev, q_host


def make_bags(rng, rows_list, B, kind, weighted):
    offs, idxs, psws = [], [], []
    for n in rows_list:
        if kind == "onehot":
            off, idx = np.arange(B, dtype=np.int64), rng.integers(0, n, size=B).astype(np.int64)
        elif kind == "empty":
            off, idx = np.zeros(B, dtype=np.int64), np.zeros(0, dtype=np.int64)
        else:
            off, idx, _ = H.ragged_bags(rng, n, B, 39 if kind == "ragged" else 4, False)
        offs.append(off); idxs.append(idx)
        psws.append(rng.uniform(-2.0, 2.0, size=idx.size).astype(np.float32) if weighted else None)
    return offs, idxs, psws


def run_and_check(bits, D, rows_list, B, kind, idx_dtype, weighted, wide, seed, tables=None, bags=None):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    T = len(rows_list)
    q_dev, q_host = tables if tables is not None else make_tables(rows_list, D, bits, seed)
    offs, idxs, psws = bags if bags is not None else make_bags(rng, rows_list, B, kind, weighted)
    bags = ops.BagBatch([to_dev(o, idx_dtype) for o in offs], [to_dev(i, idx_dtype) for i in idxs],
                        [to_dev(p) for p in psws] if weighted else None)
    CANARY = 7.5
    width = (1 + T) * D if wide else T * D
    buf = torch.full((B, width), CANARY, device=dev())
    out = buf[:, D:] if wide else buf
    ops.emb_fwd_quant(q_dev, rows_list, D, bits, bags, out)
    ops.check_index_errors(sync=True)
    first = buf.clone()
    buf2 = torch.full((B, width), CANARY, device=dev())
    ops.emb_fwd_quant(q_dev, rows_list, D, bits, bags, buf2[:, D:] if wide else buf2)
    torch.cuda.synchronize()
    assert torch.equal(first, buf2), "two runs differ"
    got = first.cpu().numpy()
    if wide:
        assert (got[:, :D] == CANARY).all(), "columns outside the embedding slots were written"
        got = got[:, D:]
    for t in range(T):
        g = got[:, t * D:(t + 1) * D]
        val, mag, L = H.dequant_sum_f64(q_host[t], bits, D, idxs[t], offs[t], psws[t])
        H.assert_within_bound(g, val, mag, L, 1.0, "table %d vs fp64" % t)
        ref = H.torch_lookup(q_host[t], bits, idxs[t], offs[t], psws[t])
        H.assert_within_bound(g, ref.astype(np.float64), mag, L, 2.0, "table %d vs torch CPU" % t)
        assert (g[L == 0] == 0).all(), "an empty bag is not zero"


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", [8, 12, 16, 64, 128, 256, 512])       # 512: 64 lanes per bag
@pytest.mark.parametrize("weighted", [False, True])
def test_lookup_one_table_ragged(bits, D, weighted):
    run_and_check(bits, D, [3000], 512, "ragged", torch.int64, weighted, wide=False, seed=100 + D + bits)


def test_lookup_33_tables_cross_the_launch_group():
    """33 8-bit tables of 7 rows, B = 5 bags of 0, 1, 5, 9 and 3 lookups: launch groups of 32 + 1; the first-row phase, one and two rounds of
    the 4-deep loop and its tail"""
    rng = np.random.default_rng(3308)
    T, rows = 33, 7
    off = np.asarray([0, 0, 1, 6, 15], dtype=np.int64)
    bags = ([off] * T, [rng.integers(0, rows, size=18).astype(np.int64) for _ in range(T)], [None] * T)
    run_and_check(8, 16, [rows] * T, 5, "ragged", torch.int64, False, wide=False, seed=3308, bags=bags)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["onehot", "ragged", "short", "empty"])
@pytest.mark.parametrize("wide", [False, True])
def test_lookup_three_tables(bits, idx_dtype, kind, wide):
    run_and_check(bits, 128, [3, 40000, 977], 1000, kind, idx_dtype, weighted=(kind == "ragged"), wide=wide, seed=200 + bits)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D,wide", [(64, True), (12, True), (12, False)])
def test_lookup_three_tables_other_dims(bits, D, wide):
    run_and_check(bits, D, [3, 5000, 100], 777, "ragged", torch.int32, True, wide=wide, seed=300 + D)


CRITEO_LIKE_ROWS = [2000000, 3, 38532, 17289, 7420, 20263, 3, 7120, 1543, 63, 2000000, 976, 14, 100000, 3, 7, 5461, 4, 10, 2208, 4, 7, 122, 3, 305, 36]


@pytest.mark.parametrize("bits", [8, 4])
def test_lookup_26_mixed_tables_at_batch_65536(bits):
    tables = make_tables(CRITEO_LIKE_ROWS, 128, bits, seed=400)
    run_and_check(bits, 128, CRITEO_LIKE_ROWS, 65536, "onehot", torch.int64, False, wide=True, seed=401, tables=tables)
    run_and_check(bits, 128, CRITEO_LIKE_ROWS, 4096, "short", torch.int32, True, wide=False, seed=402, tables=tables)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", [128, 12])
def test_out_of_range_index_is_skipped_and_reported(bits, D):
    from dlrm_amd import ops
    rng = np.random.default_rng(5)
    rows_list, B = [500, 60], 300
    q_dev, q_host = make_tables(rows_list, D, bits, seed=500)
    offs, idxs, _ = make_bags(rng, rows_list, B, "short", False)
    bad = idxs[1].size // 2
    idxs[1][bad] = rows_list[1] + 5
    idxs[0][3] = -1
    ops.check_index_errors(sync=True)
    out = torch.empty((B, 2 * D), device=dev())
    ops.emb_fwd_quant(q_dev, rows_list, D, bits, ops.BagBatch([to_dev(o) for o in offs], [to_dev(i) for i in idxs]), out)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    got = out.cpu().numpy()
    for t in range(2):
        val, mag, L = H.dequant_sum_f64(q_host[t], bits, D, idxs[t], offs[t], None, skip_out_of_range=True)
        H.assert_within_bound(got[:, t * D:(t + 1) * D], val, mag, L, 1.0, "table %d with a skipped index" % t)
    ops.check_index_errors(sync=True)            # reported once


def test_operators_refuse_wrong_operands():
    from dlrm_amd import ops
    q = ops.emb_quantize(torch.zeros((10, 16), device=dev()), 8)
    bags = ops.BagBatch([torch.arange(4, device=dev())], [torch.zeros(4, dtype=torch.int64, device=dev())])
    out = torch.empty((4, 16), device=dev())
    with pytest.raises(RuntimeError, match="packed"):
        ops.emb_fwd_quant([q], [10], 16, 4, bags, out)                   # 8-bit rows handed over as 4-bit rows
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.emb_fwd_quant([q.cpu()], [10], 16, 8, bags, out)
    with pytest.raises(RuntimeError):
        ops.emb_quantize(torch.zeros((10, 7), device=dev()), 4)          # odd dimension at 4 bits


# ------------------------------------------------------------------------------------------------ beyond 4 GiB
BIG_ROWS_Q, BIG_D = 33_000_000, 128


@pytest.fixture(scope="module")
def big_packed():
    """one 33 M x 128 table filled with the closed form of tests/test_gpu_bigtables.py, packed at 8 bits: 4.5 GB, above 2^32"""
    import test_gpu_bigtables as BT
    from dlrm_amd import ops
    free, _total = torch.cuda.mem_get_info()
    need = BIG_ROWS_Q * BIG_D * 4 + BIG_ROWS_Q * (BIG_D + 8)
    if free < need + (8 << 30):
        pytest.skip("needs %.0f GB of free HBM for the full-size table and its packed form, %.0f GB free" % (need / 1e9 + 8, free / 1e9))
    W = torch.empty((BIG_ROWS_Q, BIG_D), dtype=torch.float32, device=dev())
    BT.fill(0, W)
    q = ops.emb_quantize(W, 8)
    torch.cuda.synchronize()
    del W
    torch.cuda.empty_cache()
    assert q.numel() > 2 ** 32
    yield q
    del q
    torch.cuda.empty_cache()


def test_big_table_packed_rows_beyond_4_gib(big_packed):
    import test_gpu_bigtables as BT
    rng = np.random.default_rng(41)
    rows = BT.high_indices(rng, BIG_ROWS_Q, 4096)          # top eighth, plus row 0 and the last row
    r = to_dev(rows)
    want = H.torch_pack(BT.closed_rows(0, r).cpu().numpy(), 8)
    got = big_packed.index_select(0, r).cpu().numpy()
    assert np.array_equal(got, want)
    assert int(rows.max()) * (BIG_D + 8) > 2 ** 32


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_big_table_lookups_beyond_4_gib(big_packed, idx_dtype):
    import test_gpu_bigtables as BT
    from dlrm_amd import ops
    rng = np.random.default_rng(42)
    B = 16384
    lens = rng.integers(0, 5, size=B)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx = BT.high_indices(rng, BIG_ROWS_Q, int(lens.sum()))
    out = torch.empty((B, BIG_D), device=dev())
    ops.emb_fwd_quant([big_packed], [BIG_ROWS_Q], BIG_D, 8, ops.BagBatch([to_dev(off, idx_dtype)], [to_dev(idx, idx_dtype)]), out)
    ops.check_index_errors(sync=True)
    uniq, inv = np.unique(idx, return_inverse=True)
    small = big_packed.index_select(0, to_dev(uniq)).cpu().numpy()          # the rows the lookups name, re-indexed
    val, mag, L = H.dequant_sum_f64(small, 8, BIG_D, inv, off)
    H.assert_within_bound(out.cpu().numpy(), val, mag, L, 1.0, "33 M-row table")


# ------------------------------------------------------------------------------------------------ model
def build_model(meta, params, **kw):
    import dlrm_amd
    np.random.seed(1)
    model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                              kw.pop("interaction", "dot"), sigmoid_top=meta["sigmoid_top"], loss_function="bce", **kw)
    if params is not None:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return model


def host_params(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def forward_dev(model, X, lS_o, lS_i, idx_dtype=torch.int64):
    with torch.no_grad():
        Z = model(to_dev(X), [to_dev(o, idx_dtype) for o in lS_o], [to_dev(i, idx_dtype) for i in lS_i])
    from dlrm_amd import ops
    ops.check_index_errors(sync=True)
    return Z


def check_quantised_model(model, params, bits, X, lS_o, lS_i, **compose):
    packed_bytes = [int(e.weight.size(0)) * (e.weight.size(1) + 8 if bits == 8 else e.weight.size(1) // 2 + 4) for e in model.emb_l]
    model.quantize_embedding(bits)
    assert model.emb_l is None and model.quantize_emb is True and model.quantize_bits == bits
    assert not any(k.startswith("emb_l.") for k in model.state_dict())
    assert [q.element_size() * q.nelement() for q in model.emb_l_q] == packed_bytes
    assert all(q.is_cuda and q.dtype == torch.uint8 for q in model.emb_l_q)
    Z = forward_dev(model, X, lS_o, lS_i)
    assert Z.grad_fn is None
    want = H.torch_quant_forward(params, bits, X, lS_o, lS_i, **compose)
    np.testing.assert_allclose(Z.cpu().numpy(), want, rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
    return want


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("fixture", ["config1_b128", "kaggle_b2048", "lr_schedule_onehot_d128"])
def test_model_against_torch_operators(bits, fixture):
    d, meta = load_golden(fixture)
    model = build_model(meta, params_with_prefix(d, "init")).to(dev())
    params = host_params(model)
    T = len(meta["ln_emb"])
    X, lS_o, lS_i = d["s0.X"], [d[f"s0.off{k}"] for k in range(T)], [d[f"s0.idx{k}"] for k in range(T)]
    check_quantised_model(model, params, bits, X, lS_o, lS_i, sigmoid_top=meta["sigmoid_top"])
    # apply_emb keeps the reference's shape: one [B, D] tensor per table, no autograd node
    ly = model.apply_emb([to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i], None, model.v_W_l)
    assert len(ly) == T and all(tuple(v.shape) == (X.shape[0], meta["m_spa"]) and v.grad_fn is None for v in ly)
    packed = H.torch_pack(params["emb_l.0.weight"], bits)
    val, mag, L = H.dequant_sum_f64(packed, bits, meta["m_spa"], lS_i[0], lS_o[0])
    H.assert_within_bound(ly[0].cpu().numpy(), val, mag, L, 1.0, "apply_emb table 0")


def multihot_case(seed, D=32, B=200):
    rng = np.random.default_rng(seed)
    ln_emb = [300, 3, 4000, 17]
    F = len(ln_emb) + 1
    meta = {"m_spa": D, "ln_emb": ln_emb, "ln_bot": [13, 64, D], "ln_top": [D + F * (F - 1) // 2, 64, 1], "sigmoid_top": 1}
    X = rng.random((B, 13)).astype(np.float32)
    lS_o, lS_i = [], []
    for n in ln_emb:
        off, idx, _ = H.ragged_bags(rng, n, B, 6, False)
        lS_o.append(off); lS_i.append(idx)
    return meta, X, lS_o, lS_i


@pytest.mark.parametrize("bits", [8, 4])
def test_model_multi_hot_bags(bits):
    meta, X, lS_o, lS_i = multihot_case(61)
    model = build_model(meta, None).to(dev())
    check_quantised_model(model, host_params(model), bits, X, lS_o, lS_i, sigmoid_top=1)


@pytest.mark.parametrize("bits", [8, 4])
def test_model_fixed_pooling_weights(bits):
    meta, X, lS_o, lS_i = multihot_case(62)
    model = build_model(meta, None, weighted_pooling="fixed").to(dev())
    rng = np.random.default_rng(63)
    pool = [rng.uniform(0.25, 1.75, size=n).astype(np.float32) for n in meta["ln_emb"]]
    for k, p in enumerate(pool):
        model.v_W_l[k] = to_dev(p)
    check_quantised_model(model, host_params(model), bits, X, lS_o, lS_i, sigmoid_top=1, pool_w=pool)


@pytest.mark.parametrize("bits", [8, 4])
def test_model_cat_interaction(bits):
    meta, X, lS_o, lS_i = multihot_case(64)
    meta["ln_top"] = [meta["m_spa"] * (len(meta["ln_emb"]) + 1), 64, 1]
    model = build_model(meta, None, interaction="cat").to(dev())
    check_quantised_model(model, host_params(model), bits, X, lS_o, lS_i, sigmoid_top=1, interaction="cat")


@pytest.mark.parametrize("bits", [8, 4])
def test_model_against_the_live_reference(bits):
    d, meta = load_golden("quant_inference")
    model = build_model(meta, params_with_prefix(d, "init")).to(dev())
    model.quantize_embedding(bits)
    T = len(meta["ln_emb"])
    for s in range(meta["steps"]):
        Z = forward_dev(model, d[f"s{s}.X"], [d[f"s{s}.off{k}"] for k in range(T)], [d[f"s{s}.idx{k}"] for k in range(T)])
        np.testing.assert_allclose(Z.cpu().numpy(), d[f"pred{bits}.s{s}"], rtol=H.PRED_RTOL, atol=H.PRED_ATOL, err_msg="step %d" % s)


@pytest.mark.parametrize("bits", [8, 4])
def test_evaluate_inference_on_a_quantised_model(bits):
    from dlrm_amd import evaluate, ops
    meta, _, _, _ = multihot_case(70)
    model = build_model(meta, None).to(dev())
    params = host_params(model)
    model.quantize_embedding(bits)
    rng = np.random.default_rng(71)
    batches, preds, targets = [], [], []
    for s in range(3):
        _, X, lS_o, lS_i = multihot_case(72 + s)
        Tg = np.round(rng.random((X.shape[0], 1))).astype(np.float32)
        batches.append((torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i], torch.from_numpy(Tg)))
        preds.append(H.torch_quant_forward(params, bits, X, lS_o, lS_i, sigmoid_top=1))
        targets.append(Tg)
    got = evaluate.inference(model, batches, device=dev())
    want = ops.binary_metrics(to_dev(np.concatenate(preds).reshape(-1)), to_dev(np.concatenate(targets).reshape(-1)))
    assert set(got) == set(want)
    for k, v in want.items():
        if k in ("n", "positives", "tp", "fp", "fn", "tn"):
            assert got[k] == v, (k, got[k], v)                    # confusion counts: exactly
        else:
            assert abs(float(got[k]) - float(v)) <= 1e-6, (k, got[k], v)


# ------------------------------------------------------------------------------------------------ refusals, and the old branch
def quantised_tiny(bits=8):
    meta, X, lS_o, lS_i = multihot_case(80)
    model = build_model(meta, None).to(dev())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.quantize_embedding(bits)
    return model, opt, (X, lS_o, lS_i)


def test_distributed_forward_refuses_quantised_tables():
    model, _, (X, lS_o, lS_i) = quantised_tiny()
    with pytest.raises(SystemExit, match="ERROR: quantized embedding tables are single-process inference only"):
        model.distributed_forward(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])


def test_update_in_backward_refuses_quantised_tables():
    meta, X, lS_o, lS_i = multihot_case(81)
    model = build_model(meta, None).to(dev())
    model.update_in_backward = True
    with pytest.raises(SystemExit, match="ERROR: update_in_backward trains the embedding tables"):
        model.quantize_embedding(8)
    assert model.quantize_emb is False and model.emb_l is not None
    model.update_in_backward = False
    model.quantize_embedding(8)
    model.update_in_backward = True
    with pytest.raises(SystemExit, match="ERROR: update_in_backward trains the embedding tables"):
        model(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])


def test_stepping_an_embedding_optimizer_refuses_quantised_tables():
    model, opt, _ = quantised_tiny()
    with pytest.raises(SystemExit, match="ERROR: this optimizer holds the fp32 embedding tables"):
        opt.step()
    # an optimizer built over what the model holds NOW trains the towers only, and steps
    X, lS_o, lS_i = multihot_case(82)[1:]
    opt2 = torch.optim.SGD(model.parameters(), lr=0.1)
    Z = model(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])
    Z.sum().backward()
    opt2.step()
    torch.cuda.synchronize()


def test_graphed_train_step_refuses_a_quantised_model():
    from dlrm_amd.graph import GraphedTrainStep
    model, _, _ = quantised_tiny()
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep captures a training step"):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1))


def test_quantising_twice_is_refused():
    model, _, _ = quantised_tiny(4)
    with pytest.raises(SystemExit, match="ERROR: the embedding tables are quantized already"):
        model.quantize_embedding(8)


def test_unquantised_model_takes_the_old_branch_bit_for_bit():
    """quantize_emb == False: forward, backward and update of a deterministic-mode step, run twice from the same parameters, give the same
    bits — and so does a model on which quantize_embedding(32) (a no-op) was called"""
    from dlrm_amd import ops
    d, meta = load_golden("config1_b128")
    T = len(meta["ln_emb"])
    results = []
    for noop_call in (False, True, False):
        model = build_model(meta, params_with_prefix(d, "init")).to(dev())
        model.emb_update_mode = ops.UPD_DETERMINISTIC
        if noop_call:
            model.quantize_embedding(32)
        assert model.quantize_emb is False
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        Z = model(to_dev(d["s0.X"]), [to_dev(d[f"s0.off{k}"]) for k in range(T)], [to_dev(d[f"s0.idx{k}"]) for k in range(T)])
        E = model.loss_fn(Z, to_dev(d["s0.T"]))
        opt.zero_grad()
        E.backward()
        opt.step()
        torch.cuda.synchronize()
        results.append((Z.detach().clone(), E.detach().clone(), {k: v.clone() for k, v in model.state_dict().items()}))
    for Z, E, sd in results[1:]:
        assert torch.equal(Z, results[0][0]) and torch.equal(E, results[0][1])
        assert list(sd) == list(results[0][2]) and all(torch.equal(sd[k], results[0][2][k]) for k in sd)
