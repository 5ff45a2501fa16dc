"""Fused lookup + interaction forward over quantised tables: dlrm_interact_fwd_gather_quant / dlrm_emb_fwd_quant_pred through dlrm_amd.ops,
and DLRM_Net.fuse_quant_interact.

  * op level: R is BIT-IDENTICAL to the two-kernel form — ops.emb_fwd_quant into a feature buffer, then ops.interact_fwd over it — which is
    the reference of every equality test here; one test is independent of the project's kernels (float64 numpy from the packed bytes);
  * model level: fuse_quant_interact = True gives the prediction bits of fuse_quant_interact = False.

Live reference (tests/golden/quant_inference.npz): that fixture holds ONE configuration, m_spa = 16 with multi-hot bags (ln_emb
[60, 3, 500, 1200], 64 bags of 107-151 lookups per table).  It has no D = 128 one-hot case, so no test here runs the fused form against the
live reference's predictions; with the attribute forced on that fixture takes the two-kernel form (test_other_models_keep_the_two_kernel_form
covers that dispatch), and the bit-identity above carries the existing live-reference test over to the fused form.
"""
import numpy as np
import pytest
import torch

import test_quant_emb_host as H

pytestmark = pytest.mark.gpu

D = 128
ROWS = [1, 37, 2000, 3, 513, 1200, 2, 64, 1999, 17, 300, 5, 1024, 77, 2000, 9, 450, 31, 1500, 4, 800, 129, 11, 1777, 256, 60]      # 26 tables


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


_tables = {}


def tables(bits, T):
    """T packed tables of ROWS[t] rows from N(0, 1) weights: table 0 has a single row, table 1 (when there is one) only constant rows
    (8 bits: scale 0)"""
    from dlrm_amd import ops
    key = (bits, T)
    if key not in _tables:
        g = torch.Generator(device=dev()).manual_seed(1000 + bits)
        qs = []
        for t in range(T):
            W = torch.randn((ROWS[t], D), device=dev(), generator=g)
            if t == 1:
                W = W[:, :1].expand(-1, D).contiguous()
            qs.append(ops.emb_quantize(W, bits))
        _tables[key] = qs
    return _tables[key]


def onehot_bags(rng, rows, B, idx_dtype=torch.int64):
    from dlrm_amd import ops
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    return ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows], [to_dev(i, idx_dtype) for i in idx]), idx


def ldr_of(F, mode):
    from dlrm_amd import ops
    return (ops.interact_out_width(F, D, mode) + 3) & ~3


def guarded(B, ldr):
    """[B, ldr] view in the middle of a NaN-filled [B + 2, ldr] allocation: rows -1 and B are the canaries (the kernels fill a row up to
    ldr, its stride, with zeros: inside a row there is nothing beyond ldr)"""
    buf = torch.full((B + 2, ldr), float("nan"), device=dev())
    return buf, buf[1:B + 1]


def canaries_intact(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def two_kernel(x, qs, rows, bits, bags, mode, R):
    from dlrm_amd import ops
    B, T = x.size(0), len(qs)
    feat = torch.empty((B, (1 + T) * D), device=dev())
    feat[:, :D] = x
    if T:
        ops.emb_fwd_quant(qs, rows, D, bits, bags, feat[:, D:])
    return ops.interact_fwd((feat,), D, mode, R)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_bit_identity_grid(bits, F, idx_dtype):
    from dlrm_amd import ops
    T = F - 1
    qs, rows = tables(bits, T), ROWS[:T]
    rng = np.random.default_rng(F * 10 + bits)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = torch.randn((B, D), device=dev())
        for mode in (0, 1, 2):
            ldr = ldr_of(F, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref_buf, ref = guarded(B, ldr)
            two_kernel(x, qs, rows, bits, bags, mode, ref)
            buf1, R1 = guarded(B, ldr)
            buf2, R2 = guarded(B, ldr)
            ops.interact_fwd_gather_quant(x, qs, rows, D, bits, bags, mode, R1)
            ops.interact_fwd_gather_quant(x, qs, rows, D, bits, bags, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert same_bits(R1, ref), what
            assert same_bits(R1, R2), what + ": two runs differ"
            assert canaries_intact(buf1) and canaries_intact(buf2) and canaries_intact(ref_buf), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. full batch
@pytest.mark.parametrize("bits", [8, 4])
def test_bit_identity_full_batch(bits):
    from dlrm_amd import ops
    B, T, F = 65536, 26, 27
    g = torch.Generator(device=dev()).manual_seed(7 + bits)
    qs = [ops.emb_quantize(torch.randn((2000, D), device=dev(), generator=g), bits) for _ in range(T)]
    rows = [2000] * T
    bags, _ = onehot_bags(np.random.default_rng(bits), rows, B)
    x = torch.randn((B, D), device=dev(), generator=g)
    ldr = ldr_of(F, 0)
    ref = torch.empty((B, ldr), device=dev())
    R = torch.full((B, ldr), float("nan"), device=dev())
    two_kernel(x, qs, rows, bits, bags, 0, ref)
    ops.interact_fwd_gather_quant(x, qs, rows, D, bits, bags, 0, R)
    ops.check_index_errors(sync=True)
    assert same_bits(R, ref)


# ------------------------------------------------------------------------------------------------ 3. independent of the project's kernels
@pytest.mark.parametrize("bits", [8, 4])
def test_against_float64_numpy(bits):
    """R against a float64 product of x and the rows dequantised in numpy from the packed bytes, at the bar of
    tests/test_gpu_kernels.py::test_interact_fwd_bwd for B <= 67: rtol 1e-5, atol 1e-5.

    The data are sized for that bar, from the arithmetic and not from a run: a 128-term fp32 dot accumulates in two chains of 16 MFMA
    steps of 4 products; with unit-variance operands its partial sums reach 8-16 (ulp 1e-6), so the round-off of one output has a
    standard deviation of about 4e-6 and the worst of the 22 k outputs here (4 sigma) about 1.6e-5 — ABOVE the bar, whatever the kernel:
    N(0, 1) x N(0, 1) data would make this test a coin flip on the seed (its first run with such data missed by one element,
    1.9e-5 against 1.7e-5).  With table weights drawn N(0, 0.25^2) beside x ~ N(0, 1) every table pair's round-off is 1/16 and every
    x pair's 1/4 of that: 4 sigma = 4e-6, a factor 2.5 under the bar, while one code off by one (6 sigma_w / 255 = 6e-3 per element)
    still moves an output by hundreds of times the bar.  The oracle's element is the format's: fp32(scale * q + bias), one rounding
    (what the lookup kernel and torch's operator produce), then everything in float64."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows = ROWS[:T]
    g = torch.Generator(device=dev()).manual_seed(300 + bits)
    qs = [ops.emb_quantize(0.25 * torch.randn((n, D), device=dev(), generator=g), bits) for n in rows]
    bags, idx = onehot_bags(np.random.default_rng(33), rows, B)
    x = torch.randn((B, D), device=dev(), generator=g)
    ldr = ldr_of(F, 0)
    R = torch.empty((B, ldr), device=dev())
    ops.interact_fwd_gather_quant(x, qs, rows, D, bits, bags, 0, R)
    ops.check_index_errors(sync=True)
    feat = np.empty((B, F, D), dtype=np.float64)
    feat[:, 0] = x.cpu().numpy()
    for t in range(T):
        q, scale, bias = H.unpack(qs[t].cpu().numpy(), bits, D)
        feat[:, 1 + t] = (q * scale[:, None] + bias[:, None]).astype(np.float32)[idx[t]]
    Z = np.einsum("bid,bjd->bij", feat, feat)
    li, lj = np.tril_indices(F, -1)
    want = np.concatenate([feat[:, 0], Z[:, li, lj]], axis=1)
    got = R.cpu().numpy()
    err = np.abs(got[:, :want.shape[1]] - want)
    print("max abs error %.3g, max of error / (1e-5 + 1e-5 |want|) %.3g" % (err.max(), (err / (1e-5 + 1e-5 * np.abs(want))).max()))
    np.testing.assert_allclose(got[:, :want.shape[1]], want, rtol=1e-5, atol=1e-5)
    assert (got[:, want.shape[1]:] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. rows beyond 4 GiB
def test_rows_beyond_4_gib():
    """a 33 M-row 8-bit table (4.5 GB, never packed as a whole): only the rows the lookups name are written, taken from a small packed table"""
    import test_gpu_bigtables as BT
    from dlrm_amd import ops
    BIG, B = 33_000_000, 1000
    rng = np.random.default_rng(44)
    ids = BT.high_indices(rng, BIG, B)                         # top eighth, plus row 0 and the last row
    assert int(ids.max()) * 136 > 2 ** 32 and ids.min() == 0 and ids.max() == BIG - 1
    small = ops.emb_quantize(torch.randn((B, D), device=dev()), 8)
    big = torch.empty((BIG, 136), dtype=torch.uint8, device=dev())
    uniq = np.unique(ids)
    big.index_copy_(0, to_dev(uniq), small[:uniq.size])
    for idx_dtype in (torch.int64, torch.int32):
        bags = ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype)], [to_dev(ids, idx_dtype)])
        x = torch.randn((B, D), device=dev())
        ldr = ldr_of(2, 0)
        ref, R = torch.empty((B, ldr), device=dev()), torch.full((B, ldr), float("nan"), device=dev())
        two_kernel(x, [big], [BIG], 8, bags, 0, ref)
        ops.interact_fwd_gather_quant(x, [big], [BIG], D, 8, bags, 0, R)
        ops.check_index_errors(sync=True)
        assert same_bits(R, ref)
        # (and the rows really are the small table's: the pair column is x . dequantised row)
        q, scale, bias = H.unpack(small[:uniq.size].cpu().numpy(), 8, D)
        rowsf = (q * scale[:, None] + bias[:, None])[np.searchsorted(uniq, ids)]
        np.testing.assert_allclose(R[:, D].cpu().numpy(), (x.cpu().numpy().astype(np.float64) * rowsf).sum(1), rtol=1e-5, atol=1e-5)
    del big
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5. / 6. bad input
@pytest.mark.parametrize("bits", [8, 4])
def test_out_of_range_ids_are_reported_and_give_the_zero_row(bits):
    from dlrm_amd import ops
    B, F = 50, 4
    qs, rows = tables(bits, 3), ROWS[:3]
    rng = np.random.default_rng(5)
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    idx[1][7] = rows[1] + 3            # too large
    idx[2][31] = -1                    # negative
    offs = [torch.arange(B, device=dev()) for _ in rows]
    x = torch.randn((B, D), device=dev())
    ldr = ldr_of(F, 0)
    ops.check_index_errors(sync=True)
    ref = torch.empty((B, ldr), device=dev())
    two_kernel(x, qs, rows, bits, ops.BagBatch(offs, [to_dev(i) for i in idx]), 0, ref)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    R = torch.full((B, ldr), float("nan"), device=dev())
    ops.interact_fwd_gather_quant(x, qs, rows, D, bits, ops.BagBatch(offs, [to_dev(i) for i in idx]), 0, R)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(R, ref)
    # pairs (2, 0) and (3, 0) of the bad samples: x . zero row = +0.0
    assert R[7, D + 1].item() == 0.0 and R[31, D + 3].item() == 0.0
    ops.check_index_errors(sync=True)            # reported once


def test_broken_bag_start_is_reported():
    from dlrm_amd import ops
    B = 40
    qs, rows = tables(8, 2), ROWS[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    bags = ops.BagBatch([torch.arange(B, device=dev()), to_dev(off)], [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows])
    R = torch.empty((B, ldr_of(3, 0)), device=dev())
    ops.check_index_errors(sync=True)
    ops.interact_fwd_gather_quant(torch.randn((B, D), device=dev()), qs, rows, D, 8, bags, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 7. predicates
@pytest.mark.parametrize("bits", [8, 4])
def test_launch_predicates(bits):
    from dlrm_amd import ops
    B, F = 70, 5
    qs, rows = tables(bits, F - 1), ROWS[:F - 1]
    bags, _ = onehot_bags(np.random.default_rng(8), rows, B)
    x = torch.randn((B, D), device=dev())
    ldr = ldr_of(F, 0)
    ref = torch.empty((B, ldr), device=dev())
    two_kernel(x, qs, rows, bits, bags, 0, ref)
    E_ref = torch.empty((B, (F - 1) * D), device=dev())
    ops.emb_fwd_quant(qs, rows, D, bits, bags, E_ref)
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())
    for flag, nonzero, runs in ((zero, 0, True), (one, 1, True), (zero, 1, False), (one, 0, False)):
        R = torch.full((B, ldr), float("nan"), device=dev())
        ops.interact_fwd_gather_quant(x, qs, rows, D, bits, bags, 0, R, pred=(flag, nonzero))
        E = torch.full((B, (F - 1) * D), float("nan"), device=dev())
        ops.emb_fwd_quant(qs, rows, D, bits, bags, E, pred=(flag, nonzero))
        ops.check_index_errors(sync=True)
        if runs:
            assert same_bits(R, ref) and same_bits(E, E_ref)
        else:
            assert bool(torch.isnan(R).all()) and bool(torch.isnan(E).all())


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refused_operands():
    from dlrm_amd import ops
    B = 8
    assert ops.gather_quant_ok(27, 128, 8) and ops.gather_quant_ok(27, 128, 4) and ops.gather_quant_ok(2, 128, 8)
    assert not ops.gather_quant_ok(27, 64, 8) and not ops.gather_quant_ok(27, 128, 16) and not ops.gather_quant_ok(28, 128, 8)
    q = ops.emb_quantize(torch.randn((10, D), device=dev()), 8)
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, 0)), device=dev())
    ops.interact_fwd_gather_quant(x, [q], [10], D, 8, bags, 0, R)                       # (the operands are fine as they stand)
    # D = 64
    q64 = ops.emb_quantize(torch.randn((10, 64), device=dev()), 8)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather_quant(x[:, :64].contiguous(), [q64], [10], 64, 8, bags, 0, torch.empty((B, 68), device=dev()))
    # bits = 16
    with pytest.raises(RuntimeError, match="4 or 8 bits"):
        ops.interact_fwd_gather_quant(x, [q], [10], D, 16, bags, 0, R)
    # an unaligned packed table: a byte-offset view
    raw = torch.empty(10 * 136 + 1, dtype=torch.uint8, device=dev())
    odd = raw[1:].view(10, 136)
    odd.copy_(q)
    assert odd.data_ptr() % 8 != 0 and not ops.quant_tables_aligned([odd], 8)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather_quant(x, [odd], [10], D, 8, bags, 0, R)
    # per-sample weights
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_fwd_gather_quant(x, [q], [10], D, 8, wbags, 0, R)
    # nnz != B
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_fwd_gather_quant(x, [q], [10], D, 8, mbags, 0, R)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 9. / 10. the model
CRITEO_LIKE = [1460, 583, 2000, 1999, 305, 24, 1200, 633, 3, 931, 1500, 2000, 1890, 27, 1040, 1800, 10, 563, 201, 4, 2000, 18, 15, 1300, 105, 1420]


def criteo_model(**kw):
    import dlrm_amd
    np.random.seed(3)
    T = len(CRITEO_LIKE)
    F = T + 1
    interaction = kw.pop("interaction", "dot")
    n_top = D * F if interaction == "cat" else D + F * (F - 1) // 2
    return dlrm_amd.DLRM_Net(D, np.asarray(CRITEO_LIKE), np.asarray([13, 64, D]), np.asarray([n_top, 64, 1]), interaction,
                             sigmoid_top=1, loss_function="bce", **kw).to(dev())


def batch(seed, B=200, hots=1):
    rng = np.random.default_rng(seed)
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) * hots for _ in CRITEO_LIKE]
    lS_i = [to_dev(rng.integers(0, n, size=B * hots).astype(np.int64)) for n in CRITEO_LIKE]
    return X, lS_o, lS_i


class Counted:
    """wraps ops.interact_fwd_gather_quant / ops.emb_fwd_quant: which path did the model take"""

    def __init__(self, monkeypatch):
        from dlrm_amd import ops
        self.fused, self.lookup, self.preds = 0, 0, []
        f0, l0 = ops.interact_fwd_gather_quant, ops.emb_fwd_quant

        def fused(*a, **k):
            self.fused += 1
            self.preds.append(k.get("pred"))
            return f0(*a, **k)

        def lookup(*a, **k):
            self.lookup += 1
            return l0(*a, **k)
        monkeypatch.setattr(ops, "interact_fwd_gather_quant", fused)
        monkeypatch.setattr(ops, "emb_fwd_quant", lookup)


def forward(model, X, lS_o, lS_i, fuse):
    from dlrm_amd import ops
    model.fuse_quant_interact = fuse
    with torch.no_grad():
        Z = model(X, lS_o, lS_i)
    ops.check_index_errors(sync=True)
    assert Z.grad_fn is None
    return Z


@pytest.mark.parametrize("bits", [8, 4])
def test_model_forced_on_equals_forced_off(bits, monkeypatch):
    from dlrm_amd import ops
    model = criteo_model()
    model.quantize_embedding(bits)
    calls = Counted(monkeypatch)
    # tagged offsets: the fused kernel alone
    X, lS_o, lS_i = batch(11)
    for o in lS_o:
        ops.mark_one_lookup_per_bag(o)
    want = forward(model, X, lS_o, lS_i, False)
    assert (calls.fused, calls.lookup) == (0, 1)
    got = forward(model, X, lS_o, lS_i, True)
    assert (calls.fused, calls.lookup) == (1, 1) and calls.preds == [None]
    assert same_bits(got, want)
    # fresh untagged offsets: the device flag path — fused behind (flag, 0), the two kernels behind (flag, 1)
    X, lS_o, lS_i = batch(12)
    want = forward(model, X, lS_o, lS_i, False)
    lS_o = [o.clone() for o in lS_o]
    got = forward(model, X, lS_o, lS_i, True)
    assert (calls.fused, calls.lookup) == (2, 3) and calls.preds[-1] is not None and calls.preds[-1][1] == 0
    assert same_bits(got, want)
    # a ragged batch with nnz == B (an empty bag next to a two-lookup bag): flag path, the result is the two-kernel form's
    X, lS_o, lS_i = batch(13)
    lS_o = [o.clone() for o in lS_o]
    lS_o[4][17] = 16
    want = forward(model, X, lS_o, lS_i, False)
    lS_o = [o.clone() for o in lS_o]
    got = forward(model, X, lS_o, lS_i, True)
    assert calls.fused == 3 and calls.preds[-1] is not None
    assert same_bits(got, want)
    # fuse_emb_interact off turns the fused form off too
    model.fuse_emb_interact = False
    forward(model, X, lS_o, lS_i, True)
    assert calls.fused == 3


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("mlp_first", [False, True])
def test_model_with_quantised_towers(bits, mlp_first, monkeypatch):
    model = criteo_model()
    if mlp_first:
        model.quantize_mlp(8)
        model.quantize_embedding(bits)
    else:
        model.quantize_embedding(bits)
        model.quantize_mlp(8)
    calls = Counted(monkeypatch)
    X, lS_o, lS_i = batch(21)
    want = forward(model, X, lS_o, lS_i, False)
    got = forward(model, X, lS_o, lS_i, True)
    assert calls.fused == 1
    assert same_bits(got, want)


@pytest.mark.parametrize("bits", [8, 4])
def test_evaluate_inference_takes_the_fused_form(bits, monkeypatch):
    from dlrm_amd import evaluate
    model = criteo_model()
    model.quantize_embedding(bits)
    rng = np.random.default_rng(31)
    batches = []
    for s in range(2):
        X, lS_o, lS_i = batch(32 + s, B=150)
        Tg = torch.from_numpy(np.round(rng.random((150, 1))).astype(np.float32))
        batches.append((X.cpu(), [o.cpu() for o in lS_o], [i.cpu() for i in lS_i], Tg))
    model.fuse_quant_interact = False
    want = evaluate.inference(model, batches, device=dev())
    calls = Counted(monkeypatch)
    model.fuse_quant_interact = True
    got = evaluate.inference(model, batches, device=dev())
    assert calls.fused == 2
    assert got == want


@pytest.mark.parametrize("case", ["multihot", "cat", "pooling_weights", "gradients"])
def test_other_models_keep_the_two_kernel_form(case, monkeypatch):
    model = criteo_model(interaction="cat") if case == "cat" else criteo_model(weighted_pooling="fixed") if case == "pooling_weights" \
        else criteo_model()
    model.quantize_embedding(8)
    calls = Counted(monkeypatch)
    X, lS_o, lS_i = batch(41, hots=3 if case == "multihot" else 1)
    if case == "gradients":                   # a forward that trains the bottom tower keeps InteractFunction's autograd node
        from dlrm_amd import ops
        model.fuse_quant_interact = True
        Z = model(X, lS_o, lS_i)
        ops.check_index_errors(sync=True)
        assert Z.grad_fn is not None and (calls.fused, calls.lookup) == (0, 1)
        return
    want = forward(model, X, lS_o, lS_i, False)
    got = forward(model, X, lS_o, lS_i, True)
    assert (calls.fused, calls.lookup) == (0, 2)
    assert same_bits(got, want)
