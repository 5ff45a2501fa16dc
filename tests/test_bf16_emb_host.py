"""bfloat16 embedding tables, the part that needs no GPU:

  * numpy restatements of the two roundings the update kernels apply once per touched row (csrc/emb_bf16.hip, include/dlrm_hip.h): nearest-even,
    pinned against torch's own fp32 -> bf16 conversion, and stochastic — (bits + u) >> 16 with u 16 bits of Philox4x32-10 (oracle.philox4x32),
    counter (row lo, row hi, column / 8, 0xB0000000 | table), key = seed.  tests/test_gpu_bf16_emb.py imports them as its oracle;
  * unbiasedness of the stochastic rounding;
  * the model surface: DLRM_Net.embedding_bfloat16 / dlrm_amd.set_embedding_dtype / the launcher flag, and every refusal, each leaving the
    tables as they were.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

M64 = 2 ** 64 - 1


# ------------------------------------------------------------------------------------------------ restatements
def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_to_f32(h):
    """uint16 bit patterns -> the fp32 values they stand for (exact: a 16-bit shift)"""
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_nearest(x):
    """IEEE round-to-nearest-even of fp32 to bf16 -> uint16 bit patterns (finite and infinite inputs; NaN -> quiet NaN with the sign kept)"""
    b = f32_bits(x).astype(np.uint64)
    r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    r = np.where(nan, (b >> np.uint64(16)) | np.uint64(0x40), r)
    return r.astype(np.uint16)


def philox_u16(table, rows, D, seed):
    """the 16 random bits of every element of rows `rows` (int array [R]) of table `table`: uint32 [R, D]"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    c = np.arange(D, dtype=np.uint64).reshape(1, -1)
    w = oracle.philox4x32(rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), c >> np.uint64(3), np.uint64(0xB0000000 | int(table)), int(seed) & M64)
    wi = np.broadcast_to((c & np.uint64(7)) >> np.uint64(1), w[0].shape)
    word = np.choose(wi.astype(np.int64), [w[0], w[1], w[2], w[3]])
    odd = np.broadcast_to(c & np.uint64(1), word.shape).astype(bool)
    return np.where(odd, word >> np.uint64(16), word & np.uint64(0xFFFF)).astype(np.uint32)


def round_stochastic(x, table, rows, seed):
    """x: fp32 [R, D], the stepped rows `rows` of table `table` -> uint16 [R, D].  Finite: (bits + u) >> 16; Inf / NaN: truncated, a NaN
    stays a NaN (mantissa bit 6 set when truncation would leave none)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = f32_bits(x).astype(np.uint64)
    u = philox_u16(table, rows, x.shape[1], seed).astype(np.uint64)
    fin = ((b + u) >> np.uint64(16))
    special = (b & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    h = b >> np.uint64(16)
    h = np.where(((b & np.uint64(0x007FFFFF)) != 0) & ((h & np.uint64(0x7F)) == 0), h | np.uint64(0x40), h)
    return np.where(special, h, fin).astype(np.uint16)


def round_rows(x, mode, table, rows, seed):
    return round_nearest(x) if mode == "nearest" else round_stochastic(x, table, rows, seed)


def mix_seed(seed, call_no, stream_id=0):
    """the per-call Philox key of a model's update calls (dlrm_net._mix_seed: the mix of datagen.UniformBatchGenerator._seed)"""
    z = (seed * 0x9E3779B97F4A7C15 + call_no * 0xBF58476D1CE4E5B9 + stream_id * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z & M64


def make_bags(rng, rows, B, kind):
    """(offsets [B], indices [nnz]) int64: 'onehot' one lookup per bag; 'ragged' 0..9 lookups per bag (empty bags, the 4-deep pipeline, its tail)"""
    if kind == "onehot":
        return np.arange(B, dtype=np.int64), rng.integers(0, rows, size=B, dtype=np.int64)
    lens = rng.integers(0, 10, size=B)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return off, rng.integers(0, rows, size=int(lens.sum()), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ rounding
def test_nearest_restatement_equals_torch_on_2_pow_20_values():
    rng = np.random.default_rng(0)
    n = 1 << 20
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0x807FFFFF)          # no Inf / NaN among the random ones: they become subnormals
    k = 1 << 14
    hi = rng.integers(0, 0x7F80, size=k, dtype=np.uint64).astype(np.uint32)
    sign = rng.integers(0, 2, size=k, dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    bits[0 * k:1 * k] = sign | (hi << np.uint32(16)) | np.uint32(0x8000)      # exact ties, even and odd kept halves
    bits[1 * k:2 * k] = sign | (hi << np.uint32(16)) | np.uint32(0x7FFF)      # just below a tie
    bits[2 * k:3 * k] = sign | (hi << np.uint32(16)) | np.uint32(0x8001)      # just above
    bits[3 * k:4 * k] = sign | rng.integers(0, 1 << 23, size=k, dtype=np.uint64).astype(np.uint32)     # subnormals
    bits[4 * k:4 * k + 8] = np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0, 0x80000000], dtype=np.uint32)
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = round_nearest(x)
    assert np.array_equal(got, want)
    assert np.array_equal(bf16_to_f32(got[4 * k:4 * k + 2]), np.array([np.inf, -np.inf], dtype=np.float32))       # +-max round to +-inf


@pytest.mark.parametrize("k", [1, 16384, 32768, 65535])
def test_stochastic_rounding_is_unbiased(k):
    N, D = 1 << 20, 16
    rng = np.random.default_rng(k)
    hi = rng.integers(0x3000, 0x4000, size=N, dtype=np.uint64).astype(np.uint32)            # ordinary positive magnitudes
    x = ((hi << np.uint32(16)) | np.uint32(k)).view(np.float32).reshape(N // D, D)
    got = round_stochastic(x, 3, np.arange(N // D), seed=0x1234ABCD5678)
    up = got.reshape(-1).astype(np.int64) - hi.astype(np.int64)
    assert set(np.unique(up)) <= {0, 1}
    f = k / 65536.0
    share = float(up.mean())
    print("k = %d: share rounded up %.6f, expected %.6f, bound %.6f" % (k, share, f, 6 * np.sqrt(f * (1 - f) / N)))
    assert abs(share - f) <= 6 * np.sqrt(f * (1 - f) / N)


def test_stochastic_rounding_never_changes_representable_values_and_keeps_specials():
    N, D = 1 << 20, 16
    rng = np.random.default_rng(7)
    hi = rng.integers(0, 0x10000, size=N, dtype=np.uint64).astype(np.uint32)
    hi[(hi & 0x7F80) == 0x7F80] = 0x3F80
    x = (hi << np.uint32(16)).view(np.float32).reshape(N // D, D)
    got = round_stochastic(x, 0, np.arange(N // D), seed=99)
    assert np.array_equal(got.reshape(-1), hi.astype(np.uint16))
    sp = np.array([[0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFF80FFFF, 0x7FFFFFFF, 0x7F7FFFFF, 0x7F7F0000]], dtype=np.uint32).view(np.float32)
    h = round_stochastic(sp, 0, [5], seed=1)[0]
    assert h[0] == 0x7F80 and h[1] == 0xFF80 and h[2] == 0x7FC0 and h[3] == 0x7FC0 and h[4] == 0xFFC0 and h[5] == 0x7FFF
    assert h[6] in (0x7F7F, 0x7F80) and h[7] == 0x7F7F          # a carry out of the largest finite value is +inf; a representable one stays
    assert np.isnan(bf16_to_f32(h[2:6])).all()


def test_stream_depends_on_seed_table_row_and_column_only():
    a = philox_u16(2, [7, 1 << 33], 24, seed=5)
    assert np.array_equal(a, philox_u16(2, [7, 1 << 33], 24, seed=5))
    assert not np.array_equal(a, philox_u16(2, [7, 1 << 33], 24, seed=6))
    assert not np.array_equal(a, philox_u16(3, [7, 1 << 33], 24, seed=5))
    assert np.array_equal(a[:, :8], philox_u16(2, [7, 1 << 33], 8, seed=5))        # independent of D
    assert not np.array_equal(a[0], a[1])
    w = oracle.philox4x32(7, 0, 2, 0xB0000002, 5)                                   # columns 16 .. 23 of row 7: block 2
    assert a[0, 16] == int(w[0]) & 0xFFFF and a[0, 17] == int(w[0]) >> 16 and a[0, 23] == int(w[3]) >> 16


# ------------------------------------------------------------------------------------------------ model surface
def tiny_model(**kw):
    import dlrm_amd
    np.random.seed(11)
    torch.manual_seed(11)
    return dlrm_amd.DLRM_Net(8, np.asarray([300, 7, 3]), np.asarray([13, 8]), np.asarray([14, 1]), "dot", sigmoid_top=0, **kw)


def tables_of(model):
    return [(w, w.dtype, w.detach().clone()) for w in model._emb_weights(model.emb_l)]


def assert_untouched(snap, model):
    now = model._emb_weights(model.emb_l)
    assert len(now) == len(snap)
    for (w, dt, val), cur in zip(snap, now):
        assert cur is w and cur.dtype == dt and torch.equal(cur.detach(), val)


def test_conversion_keeps_parameters_keys_and_rounds_to_nearest():
    model = tiny_model()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = [p for p in model.parameters()]
    keys = list(model.state_dict())
    fp32 = [e.weight.detach().clone() for e in model.emb_l]
    model.embedding_bfloat16("nearest", seed=5)
    after = [p for p in model.parameters()]
    assert len(before) == len(after) and all(a is b for a, b in zip(before, after))
    assert all(any(p is e.weight for g in opt.param_groups for p in g["params"]) for e in model.emb_l)
    sd = model.state_dict()
    assert list(sd) == keys
    for k, v in sd.items():
        assert v.dtype == (torch.bfloat16 if k.startswith("emb_l.") else torch.float32), k
    for e, w in zip(model.emb_l, fp32):
        got = e.weight.detach().view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, round_nearest(w.numpy()))
    assert model.emb_bf16 == ("nearest", 5)


def test_loading_an_fp32_checkpoint_casts():
    a, b = tiny_model(), tiny_model()
    b.embedding_bfloat16()
    sd = {k: (v + 0.001 if k.startswith("emb_l.") else v) for k, v in a.state_dict().items()}
    b.load_state_dict(sd)
    for k, v in b.state_dict().items():
        if k.startswith("emb_l."):
            assert v.dtype == torch.bfloat16 and torch.equal(v, sd[k].to(torch.bfloat16))


def test_update_seeds_follow_the_generator_mix():
    model = tiny_model()
    model.embedding_bfloat16("stochastic", seed=42)
    assert [model._bf16_next_seed() for _ in range(3)] == [mix_seed(42, n) for n in range(3)]
    assert len({mix_seed(42, n) for n in range(100)} | {mix_seed(43, n) for n in range(100)}) == 200


def test_set_embedding_dtype_creates_bf16_tables():
    import dlrm_amd
    ref = tiny_model()
    dlrm_amd.set_embedding_dtype(torch.bfloat16, "nearest", 9)
    try:
        model = tiny_model()
    finally:
        dlrm_amd.set_embedding_dtype(None)
    assert model.emb_bf16 == ("nearest", 9)
    for e, r in zip(model.emb_l, ref.emb_l):
        assert e.weight.dtype == torch.bfloat16 and torch.equal(e.weight.detach(), r.weight.detach().to(torch.bfloat16))
    assert tiny_model().emb_bf16 is None and tiny_model().emb_l[0].weight.dtype == torch.float32
    with pytest.raises(SystemExit, match="ERROR: embedding tables are float32 or bfloat16"):
        dlrm_amd.set_embedding_dtype(torch.float16)
    with pytest.raises(SystemExit, match="ERROR: bfloat16 embedding tables round 'stochastic' or 'nearest'"):
        dlrm_amd.set_embedding_dtype(torch.bfloat16, "up")


def test_set_embedding_dtype_refuses_qr_and_md_models_before_building_tables():
    import dlrm_amd
    dlrm_amd.set_embedding_dtype(torch.bfloat16)
    try:
        with pytest.raises(SystemExit, match="ERROR: bfloat16 embedding tables with quotient remainder are not supported"):
            tiny_model(qr_flag=True, qr_collisions=4, qr_threshold=100)
        with pytest.raises(SystemExit, match="ERROR: bfloat16 embedding tables with learned pooling weights are not supported"):
            tiny_model(weighted_pooling="learned")
    finally:
        dlrm_amd.set_embedding_dtype(None)


def test_launcher_flag_is_parsed():
    from dlrm_amd import launch
    a = launch.build_parser().parse_args(["--bf16-tables", "nearest", "--bf16-seed", "7"])
    assert a.bf16_tables == "nearest" and a.bf16_seed == 7
    assert launch.build_parser().parse_args(["--bf16-tables", "stochastic"]).bf16_tables == "stochastic"
    assert launch.build_parser().parse_args([]).bf16_tables is None
    with pytest.raises(SystemExit):
        launch.build_parser().parse_args(["--bf16-tables", "truncate"])


def _refused(model, match, call):
    snap = tables_of(model)
    with pytest.raises(SystemExit, match=match):
        call()
    assert_untouched(snap, model)


def test_refuses_an_unknown_rounding():
    model = tiny_model()
    _refused(model, "ERROR: bfloat16 embedding tables round 'stochastic' or 'nearest'", lambda: model.embedding_bfloat16("truncate"))
    assert model.emb_bf16 is None


def test_refuses_qr_tables():
    model = tiny_model(qr_flag=True, qr_collisions=4, qr_threshold=100)
    _refused(model, "ERROR: bfloat16 embedding tables with quotient remainder are not supported", model.embedding_bfloat16)


def test_refuses_md_tables():
    import dlrm_amd
    model = dlrm_amd.DLRM_Net([8, 4, 8], np.asarray([300, 250, 3]), np.asarray([13, 8]), np.asarray([14, 1]), "dot", md_flag=True, md_threshold=200)
    _refused(model, "ERROR: bfloat16 embedding tables with mixed dimensions are not supported", model.embedding_bfloat16)


def test_refuses_learned_pooling_weights_and_accepts_fixed_ones():
    model = tiny_model(weighted_pooling="learned")
    _refused(model, "ERROR: bfloat16 embedding tables with learned pooling weights are not supported", model.embedding_bfloat16)
    fixed = tiny_model(weighted_pooling="fixed")
    fixed.embedding_bfloat16()
    assert fixed.emb_l[0].weight.dtype == torch.bfloat16


def test_refuses_the_coo_gradient_path():
    model = tiny_model()
    model.fused_emb_update = False
    _refused(model, "ERROR: bfloat16 embedding tables need the fused embedding update", model.embedding_bfloat16)
    model = tiny_model()
    model.embedding_bfloat16()
    model.fused_emb_update = False                 # switched off after the conversion: refused where the gradient arrives
    ws = tuple(model._emb_weights(model.emb_l))
    _refused(model, "ERROR: bfloat16 embedding tables need the fused embedding update", lambda: model._stash_embedding_grad(ws, None, None))
    model.fused_emb_update = True
    opt = torch.optim.Adam(model.parameters(), lr=0.1)       # an optimizer the fused kernels do not implement: the ("coo",) plan
    _refused(model, "ERROR: bfloat16 embedding tables are updated by the fused kernels only", lambda: model._apply_pending([(ws, None, None, None)], opt, None))
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    _refused(model, "ERROR: bfloat16 embedding tables are updated by the fused kernels only", lambda: model._apply_pending([(ws, None, None, None)], opt, None))


def test_refuses_quantize_embedding_both_ways():
    model = tiny_model()
    model.embedding_bfloat16()
    _refused(model, "ERROR: 4 and 8-bit quantization with bfloat16 embedding tables is not supported", lambda: model.quantize_embedding(8))
    assert model.quantize_emb is False


def test_refuses_distributed_forward():
    model = tiny_model()
    model.embedding_bfloat16()
    _refused(model, "ERROR: bfloat16 embedding tables are single-process only",
             lambda: model.distributed_forward(torch.zeros((2, 13)), [torch.zeros(2, dtype=torch.int64)] * 3, [torch.zeros(2, dtype=torch.int64)] * 3))


def test_refuses_graphed_train_step():
    from dlrm_amd.graph import GraphedTrainStep
    model = tiny_model()
    model.embedding_bfloat16()
    _refused(model, "ERROR: GraphedTrainStep is not built for bfloat16 embedding tables",
             lambda: GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1)))


def test_refuses_the_torchrec_variants():
    from dlrm_amd import torchrec_variant as tv
    model = tv.DLRM([300, 7, 3], 8, 13, [16, 8], [16, 1])
    _refused(model, "ERROR: bfloat16 embedding tables are built for DLRM_Net only, not for the torchrec variants", model.embedding_bfloat16)
    for cls in (tv.DLRM, tv.ShardedDLRM, tv.DLRM_DCN):
        assert cls._bf16_supported is False


def test_refuses_converting_twice_and_converting_with_a_parked_update():
    model = tiny_model()
    model._pending_emb.append(("parked",))
    _refused(model, "ERROR: an embedding update is still parked", model.embedding_bfloat16)
    model._pending_emb.clear()
    model.embedding_bfloat16()
    _refused(model, "ERROR: the embedding tables are bfloat16 already", model.embedding_bfloat16)
