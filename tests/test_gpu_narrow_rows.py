"""Fused lookup + interaction over bfloat16 tables (forward and backward) and over 8- / 4-bit packed tables (forward) of D = 16 / 32 / 64:
dlrm_interact_{fwd,bwd}_gather_narrow_bf16 and dlrm_interact_fwd_gather_narrow_quant through dlrm_amd.ops, and the model paths that
DLRM_Net.fuse_narrow_interact opens together with fuse_bf16_interact / fuse_quant_interact.

  * op level: R, dx, dE are BIT-IDENTICAL to the two-kernel form (ops.emb_fwd_bf16 / ops.emb_fwd_quant into a feature buffer, then
    ops.interact_fwd / ops.interact_bwd over it) — never to the kernels under test; one test is independent of the project's kernels
    (float64 numpy on exactly upcast / dequantised inputs, the bounds of tests/test_gpu_narrow_interact.py::test_against_float64_numpy);
  * model level: the flags on give the prediction bits, the loss and — after one optimizer step — the table bits, the Adagrad accumulators
    and the tower parameters of the flags off.

Batch sizes: a workgroup has four waves and a wave takes one sample per pass, so B = 1 leaves three waves of the only workgroup without a
sample, B = 5 gives the first wave of a second workgroup one sample (every look-ahead of every wave is clamped at B - 1), and B = 300 needs
75 workgroups.  Tables have at most 2000 rows; table 0 has one row, table 3 three.
"""
import numpy as np
import pytest
import torch

import test_quant_emb_host as H

pytestmark = pytest.mark.gpu

ROWS = [1, 37, 2000, 3, 513, 1200, 2, 64, 1999, 17, 300, 5, 1024, 77, 2000, 9, 450, 31, 1500, 4, 800, 129, 11, 1777, 256, 60,
        700, 13, 1999, 90, 333]      # 31 tables: F = 32 is the widest shape the kernels take
BATCHES = (1, 5, 300)
KINDS = ("bf16", "q8", "q4")
# bfloat16 bit patterns: -0.0, subnormals of both signs, +0.0, the smallest normal
SPECIAL16 = np.array([0x8000, 0x0001, 0x8001, 0x007F, 0x0040, 0x807F, 0x0000, 0x0080], dtype=np.uint16)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    return np.array_equal(a.detach().contiguous().cpu().numpy().view(np.int32), b.detach().contiguous().cpu().numpy().view(np.int32))


def bits16(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def upcast(bits):
    """bfloat16 bit patterns (uint16) -> the fp32 values they stand for, exactly"""
    return (bits.astype(np.uint32) << 16).view(np.float32)


_tables = {}


def tables(kind, T, D):
    """(device tables, their rows as fp32 numpy arrays — exactly what a lookup of one row widens / dequantises to, before the +0.0 add).
    bf16: uniform in [-1, 1] rounded to bfloat16; the single row of table 0 carries -0.0 and subnormals in its first columns, the first ten
    rows of table 1 consist of them.  Packed: N(0, 1) weights through ops.emb_quantize; table 1 has only constant rows (8 bits: scale 0)."""
    from dlrm_amd import ops
    key = (kind, D)
    if key not in _tables:
        rng = np.random.default_rng(77 + D)
        ws, hs = [], []
        for t, n in enumerate(ROWS):
            if kind == "bf16":
                b = bits16(to_dev(rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32)).to(torch.bfloat16)).view(np.uint16).copy()
                if t == 0:
                    b[0, :SPECIAL16.size] = SPECIAL16
                if t == 1:
                    b[:10] = np.tile(SPECIAL16, D // SPECIAL16.size)[None, :]
                ws.append(to_dev(b.view(np.int16)).view(torch.bfloat16))
                hs.append(upcast(b))
            else:
                bits = 8 if kind == "q8" else 4
                W = to_dev(rng.standard_normal((n, D)).astype(np.float32))
                if t == 1:
                    W = W[:, :1].expand(-1, D).contiguous()
                q = ops.emb_quantize(W, bits)
                ws.append(q)
                hs.append(dequantised(q, bits, D))
        _tables[key] = (ws, hs)
    ws, hs = _tables[key]
    return ws[:T], hs[:T]


def dequantised(q, bits, D):
    """fp32(scale * code + bias), one rounding: the format's element (the float64 product and sum are exact to 2^-53, then rounded once)"""
    code, scale, bias = H.unpack(q.cpu().numpy(), bits, D)
    return (code * scale[:, None] + bias[:, None]).astype(np.float32)


def bits_of_kind(kind):
    return {"q8": 8, "q4": 4}.get(kind)


def onehot_bags(rng, rows, B, idx_dtype=torch.int64):
    from dlrm_amd import ops
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    return ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows], [to_dev(i, idx_dtype) for i in idx]), idx


def ldr_of(F, D, mode):
    from dlrm_amd import ops
    return (ops.interact_out_width(F, D, mode) + 3) & ~3


def guarded(B, w):
    """[B, w] column view (row pitch w + 8) in the middle of a NaN-filled [B + 2, w + 8] allocation"""
    buf = torch.full((B + 2, w + 8), float("nan"), device=dev())
    return buf, buf[1:B + 1, 4:4 + w]


def guarded_rows(B, ld):
    buf = torch.full((B + 2, ld), float("nan"), device=dev())
    return buf, buf[1:B + 1]


def row_canaries_intact(*bufs):
    return all(bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[-1]).all()) for b in bufs)


def canaries_intact(*bufs):
    return all(bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[-1]).all()) and bool(torch.isnan(b[:, :4]).all())
               and bool(torch.isnan(b[:, -4:]).all()) for b in bufs)


def wide(t):
    buf = torch.full((t.size(0), t.size(1) + 8), 123.0, device=t.device)
    v = buf[:, 4:4 + t.size(1)]
    v.copy_(t)
    return v


def pooled(kind, ws, rows, bags, B, D, pred=None):
    """the [B, T*D] fp32 buffer of the two-kernel form"""
    from dlrm_amd import ops
    E = torch.full((B, len(ws) * D), -7.0, device=dev())
    if kind == "bf16":
        ops.emb_fwd_bf16(ws, bags, E, pred=pred)
    else:
        ops.emb_fwd_quant(ws, rows, D, bits_of_kind(kind), bags, E, pred=pred)
    return E


def fused_fwd(kind, x, ws, rows, bags, D, mode, R, pred=None):
    from dlrm_amd import ops
    if kind == "bf16":
        return ops.interact_fwd_gather_narrow_bf16(x, ws, bags, D, mode, R, pred=pred)
    return ops.interact_fwd_gather_narrow_quant(x, ws, rows, D, bits_of_kind(kind), bags, mode, R, pred=pred)


def x_with_zeros_and_negatives(B, D):
    x = torch.randn((B, D), device=dev())
    x[:, 5::16] = 0.0
    return x


def dR_of(B, F, D, mode):
    from dlrm_amd import ops
    Wd = ops.interact_out_width(F, D, mode)
    dR = torch.zeros((B, ldr_of(F, D, mode)), device=dev())
    dR[:, :Wd] = torch.randn((B, Wd), device=dev())
    return dR


# ------------------------------------------------------------------------------------------------ 1. the forward grid
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27, 32])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_bit_identity_grid(kind, D, F, idx_dtype):
    """F = 16 / 17 straddle the NB = 1 / 2 instantiations, F = 32 fills every feature slot"""
    from dlrm_amd import ops
    T = F - 1
    ws, hs = tables(kind, T, D)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10 + D)
    ops.check_index_errors(sync=True)
    for B in BATCHES:
        bags, idx = onehot_bags(rng, rows, B, idx_dtype)
        if B == 300 and kind == "bf16" and T >= 2:
            assert (idx[1] < 10).any() and hs[1][0, 0] == 0 and np.signbit(hs[1][0, 0])      # rows with -0.0 entries are looked up
        x = torch.randn((B, D), device=dev())
        E = pooled(kind, ws, rows, bags, B, D)
        for mode in (0, 1, 2):
            ldr = ldr_of(F, D, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref = torch.empty((B, ldr), device=dev())
            ops.interact_fwd((x, E), D, mode, ref)
            buf1, R1 = guarded_rows(B, ldr)
            buf2, R2 = guarded_rows(B, ldr)
            fused_fwd(kind, x, ws, rows, bags, D, mode, R1)
            fused_fwd(kind, x, ws, rows, bags, D, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert np.array_equal(R1.cpu().numpy().view(np.int32), ref.cpu().numpy().view(np.int32)), what + ": the two-kernel form"
            assert same_bits(R1, R2), what + ": two runs differ"
            assert row_canaries_intact(buf1, buf2), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. the backward grid (bf16)
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27, 32])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_backward_bit_identity_grid(D, F, idx_dtype):
    """the axes of the forward grid; x, dR, dx, dE are column views of wider allocations (ld = width + 8); with and without INTERACT_RELU_X"""
    from dlrm_amd import ops
    T = F - 1
    ws, _ = tables("bf16", T, D)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10 + D + 1)
    ops.check_index_errors(sync=True)
    for B in BATCHES:
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = wide(x_with_zeros_and_negatives(B, D))
        assert x.stride(0) == D + 8
        E = pooled("bf16", ws, rows, bags, B, D)
        for mode in (0, 1, 2):
            dR = wide(dR_of(B, F, D, mode))
            for relu in (0, ops.INTERACT_RELU_X):
                m = mode | relu
                dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
                ops.interact_bwd((x, E), D, m, dR, (dx_ref, dE_ref))
                outs = []
                for _ in range(2):
                    bx, dx = guarded(B, D)
                    be, dE = guarded(B, T * D)
                    ops.interact_bwd_gather_narrow_bf16(x, ws, bags, D, m, dR, dx, dE)
                    outs.append((bx, dx, be, dE))
                ops.check_index_errors(sync=True)
                (bx, dx, be, dE), (bx2, dx2, be2, dE2) = outs
                what = "B=%d mode=%d relu=%d" % (B, mode, relu)
                assert not torch.isnan(dx).any() and not torch.isnan(dE).any(), what
                assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref), what + ": the two-kernel form"
                assert same_bits(dx, dx2) and same_bits(dE, dE2), what + ": two runs differ"
                assert canaries_intact(bx, be, bx2, be2), what
                if relu:
                    assert bool((dx[x <= 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------ 3. independent of the project's kernels
@pytest.mark.parametrize("D", [16, 32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_against_float64_numpy(kind, D):
    """R (and, bf16, dx and dE) against float64 numpy on rows widened / dequantised in numpy, within the any-order fp32 summation bounds of
    tests/test_gpu_narrow_interact.py::test_against_float64_numpy (u = 2^-24):
    forward pair (a, b): |err| <= (D + 1) u sum_k |a_k| |b_k|;  backward: |err| <= (F + 2) u (sum_j |S_ij| |T_jd| + |dR_d|), the dR_d term for
    feature 0 only."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows = ROWS[:T]
    rng = np.random.default_rng(303 + D)
    # (normal data without subnormals, as the fp32 test: the bound is relative to sum |a| |b|)
    if kind == "bf16":
        ws = [to_dev(rng.standard_normal((n, D)).astype(np.float32)).to(torch.bfloat16) for n in rows]
        hs = [upcast(bits16(w).view(np.uint16)) for w in ws]
    else:
        ws = [ops.emb_quantize(to_dev(rng.standard_normal((n, D)).astype(np.float32)), bits_of_kind(kind)) for n in rows]
        hs = [dequantised(q, bits_of_kind(kind), D) for q in ws]
    bags, idx = onehot_bags(np.random.default_rng(33), rows, B)
    xn = rng.standard_normal((B, D)).astype(np.float32)
    x = to_dev(xn)
    Wd = ops.interact_out_width(F, D, 0)
    ldr = ldr_of(F, D, 0)
    R = torch.empty((B, ldr), device=dev())
    fused_fwd(kind, x, ws, rows, bags, D, 0, R)
    ops.check_index_errors(sync=True)
    feat = np.empty((B, F, D), dtype=np.float64)
    feat[:, 0] = xn
    for t in range(T):
        feat[:, 1 + t] = hs[t][idx[t]]
    u = 2.0 ** -24
    li, lj = np.tril_indices(F, -1)
    Z = np.einsum("bik,bjk->bij", feat, feat)
    Zabs = np.einsum("bik,bjk->bij", np.abs(feat), np.abs(feat))
    got = R.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, :D], xn.astype(np.float64))
    assert (got[:, Wd:] == 0).all()
    err_f = np.abs(got[:, D:Wd] - Z[:, li, lj])
    bound_f = (D + 1) * u * Zabs[:, li, lj]
    print("forward: worst error / bound %.3g" % float((err_f / np.maximum(bound_f, 1e-300)).max()))
    assert (err_f <= bound_f).all()
    if kind != "bf16":
        return
    dRn = rng.standard_normal((B, Wd)).astype(np.float32)
    dR = torch.zeros((B, ldr), device=dev())
    dR[:, :Wd] = to_dev(dRn)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd_gather_narrow_bf16(x, ws, bags, D, 0, dR, dx, dE)
    ops.check_index_errors(sync=True)
    S = np.zeros((B, F, F))
    S[:, li, lj] = dRn[:, D:].astype(np.float64)
    S[:, lj, li] = dRn[:, D:].astype(np.float64)
    dT = np.einsum("bij,bjd->bid", S, feat)
    dTabs = np.einsum("bij,bjd->bid", np.abs(S), np.abs(feat))
    dT[:, 0] += dRn[:, :D]
    dTabs[:, 0] += np.abs(dRn[:, :D])
    gotT = np.concatenate([dx.cpu().numpy()[:, None, :], dE.cpu().numpy().reshape(B, T, D)], axis=1).astype(np.float64)
    err_b = np.abs(gotT - dT)
    bound_b = (F + 2) * u * dTabs
    print("backward: worst error / bound %.3g" % float((err_b / np.maximum(bound_b, 1e-300)).max()))
    assert (err_b <= bound_b).all()


# ------------------------------------------------------------------------------------------------ 4. bad input
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_out_of_range_ids_are_reported_and_give_the_zero_row(kind, D, idx_dtype):
    """ids that are negative, equal to `rows` and very large: reported, a row of +0.0; every other sample has the bits of a clean run"""
    from dlrm_amd import ops
    B, F = 50, 4
    ws, _ = tables(kind, 3, D)
    rows = ROWS[:3]
    rng = np.random.default_rng(5)
    clean = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    idx = [c.copy() for c in clean]
    idx[1][7] = rows[1]                                              # equal to rows
    idx[2][31] = -1                                                  # negative
    idx[0][44] = 2 ** 31 - 1 if idx_dtype == torch.int32 else 2 ** 40 + 5      # very large
    bad = [7, 31, 44]
    good = [b for b in range(B) if b not in bad]
    offs = [torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows]

    def bags(ids):
        return ops.BagBatch(offs, [to_dev(i, idx_dtype) for i in ids])
    x = x_with_zeros_and_negatives(B, D)
    x[:, 0] = 1.0
    ldr = ldr_of(F, D, 0)
    ops.check_index_errors(sync=True)
    # the two-kernel form: its lookup reports the same ids
    E = pooled(kind, ws, rows, bags(idx), B, D)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E), D, 0, ref)
    E_clean = pooled(kind, ws, rows, bags(clean), B, D)
    ref_clean = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_clean), D, 0, ref_clean)
    ops.check_index_errors(sync=True)
    # forward
    R = torch.full((B, ldr), float("nan"), device=dev())
    fused_fwd(kind, x, ws, rows, bags(idx), D, 0, R)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(R, ref)
    assert same_bits(R[good], ref_clean[good])
    # pairs (f, 0) of the bad samples: x . zero row = +0.0 (positions: (1,0) = D, (2,0) = D + 1, (3,0) = D + 3)
    zero_bits = R[[7, 31, 44], [D + 1, D + 3, D]].view(torch.int32)
    assert bool((zero_bits == 0).all())
    ops.check_index_errors(sync=True)            # reported once
    if kind != "bf16":
        return
    # backward: the gradient row of the bad lookup is written like any other
    dR = dR_of(B, F, D, 0)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd((x, E), D, 0, dR, (dx_ref, dE_ref))
    dx_c, dE_c = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd((x, E_clean), D, 0, dR, (dx_c, dE_c))
    dx, dE = torch.full((B, D), float("nan"), device=dev()), torch.full((B, 3 * D), float("nan"), device=dev())
    ops.interact_bwd_gather_narrow_bf16(x, ws, bags(idx), D, 0, dR, dx, dE)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert not torch.isnan(dE).any() and not torch.isnan(dx).any()
    assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
    assert same_bits(dx[good], dx_c[good]) and same_bits(dE[good], dE_c[good])
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_broken_bag_start_is_reported(kind, D):
    from dlrm_amd import ops
    B = 40
    ws, _ = tables(kind, 2, D)
    rows = ROWS[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    ids = [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows]
    broken = ops.BagBatch([torch.arange(B, device=dev()), to_dev(off)], ids)
    clean = ops.BagBatch([torch.arange(B, device=dev()), torch.arange(B, device=dev())], ids)
    x = torch.randn((B, D), device=dev())
    ldr = ldr_of(3, D, 0)
    R, Rc = torch.full((B, ldr), float("nan"), device=dev()), torch.empty((B, ldr), device=dev())
    ops.check_index_errors(sync=True)
    fused_fwd(kind, x, ws, rows, clean, D, 0, Rc)
    ops.check_index_errors(sync=True)
    fused_fwd(kind, x, ws, rows, broken, D, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    others = [b for b in range(B) if b != 11]
    assert same_bits(R[others], Rc[others]) and not torch.isnan(R).any()
    if kind == "bf16":
        dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, 2 * D), device=dev())
        ops.interact_bwd_gather_narrow_bf16(x, ws, broken, D, 0, dR_of(B, 3, D, 0), dx, dE)
        with pytest.raises(IndexError, match="does not start at its own position"):
            ops.check_index_errors(sync=True)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 5. row offsets beyond 4 GiB
def test_rows_beyond_4_gib():
    """a bf16 table of just over 2^25 rows of D = 64 (128 bytes each: 4 GiB + 512 KiB, never filled): only the rows the lookups name are
    written, in closed form.  Values k / 64 with |k| <= 125 and x of small integers make every product and every partial sum exact in fp32, so
    the pair column must EQUAL the float64 dot product."""
    from dlrm_amd import ops
    D, B = 64, 300
    BIG = 2 ** 25 + 4096
    rng = np.random.default_rng(44)
    # half of the ids from the top eighth (below 4 GiB), half from the 4096 rows whose byte offset does not fit 32 bits
    ids = np.where(np.arange(B) % 2 == 0, rng.integers(BIG - BIG // 8, 2 ** 25, size=B), rng.integers(2 ** 25, BIG, size=B)).astype(np.int64)
    ids[0], ids[1], ids[2], ids[3], ids[-1] = BIG - 1, 0, 2 ** 25, 2 ** 25 - 1, BIG - 1
    assert int(ids.max()) * 2 * D >= 2 ** 32 and (ids * 2 * D >= 2 ** 32).sum() >= B // 2 and ids.min() == 0
    uniq = np.unique(ids)
    vals = (((uniq[:, None] * 31 + np.arange(D)[None, :] * 7) % 251) - 125).astype(np.float32) / 64.0
    big = torch.empty((BIG, D), dtype=torch.bfloat16, device=dev())
    big.index_copy_(0, to_dev(uniq), to_dev(vals).to(torch.bfloat16))
    assert np.array_equal(big[to_dev(uniq)].float().cpu().numpy(), vals)          # exactly representable
    xn = rng.integers(-4, 5, size=(B, D)).astype(np.float32)
    x = to_dev(xn)
    want = (xn.astype(np.float64) * vals[np.searchsorted(uniq, ids)].astype(np.float64)).sum(1)
    ldr = ldr_of(2, D, 0)
    dRn = rng.integers(-3, 4, size=(B, ldr)).astype(np.float32)
    dRn[:, D + 1:] = 0.0
    dR = to_dev(dRn)
    ops.check_index_errors(sync=True)
    for idx_dtype in (torch.int64, torch.int32):
        bags = ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype)], [to_dev(ids, idx_dtype)])
        E = torch.empty((B, D), device=dev())
        ops.emb_fwd_bf16([big], bags, E)
        ref, R = torch.empty((B, ldr), device=dev()), torch.full((B, ldr), float("nan"), device=dev())
        ops.interact_fwd((x, E), D, 0, ref)
        ops.interact_fwd_gather_narrow_bf16(x, [big], bags, D, 0, R)
        ops.check_index_errors(sync=True)
        assert same_bits(R, ref)
        assert np.array_equal(R[:, D].cpu().numpy().astype(np.float64), want)
        # backward: dE = dZ * x exactly; dx = dR_x + dZ * row
        dx, dE = torch.full((B, D), float("nan"), device=dev()), torch.full((B, D), float("nan"), device=dev())
        ops.interact_bwd_gather_narrow_bf16(x, [big], bags, D, 0, dR, dx, dE)
        ops.check_index_errors(sync=True)
        dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, D), device=dev())
        ops.interact_bwd((x, E), D, 0, dR, (dx_ref, dE_ref))
        assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
        rowsn = vals[np.searchsorted(uniq, ids)].astype(np.float64)
        assert np.array_equal(dx.cpu().numpy().astype(np.float64), dRn[:, :D] + dRn[:, D:D + 1].astype(np.float64) * rowsn)
        assert np.array_equal(dE.cpu().numpy().astype(np.float64), dRn[:, D:D + 1].astype(np.float64) * xn)
    del big
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 6. launch predicates
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_launch_predicates(kind, D):
    """with (flag, 0) / (flag, 1) exactly one of the fused form and the two-kernel form writes R (and, bf16, dx / dE): the launch that must
    not run leaves its -7.0-filled output untouched, the other gives the unpredicated bits"""
    from dlrm_amd import ops
    B, F = 70, 5
    T = F - 1
    ws, _ = tables(kind, T, D)
    rows = ROWS[:T]
    bags, _ = onehot_bags(np.random.default_rng(8), rows, B)
    x = x_with_zeros_and_negatives(B, D)
    ldr = ldr_of(F, D, 0)
    dR = dR_of(B, F, D, 0)
    E_ref = pooled(kind, ws, rows, bags, B, D)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_ref), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E_ref), D, 0, dR, (dx_ref, dE_ref))
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())

    def filled(*shape):
        return torch.full(shape, -7.0, device=dev())

    def untouched(*ts):
        return all(bool((t == -7.0).all()) for t in ts)
    for flag in (zero, one):
        fused_runs = flag is zero                      # the fused form goes behind (flag, 0), the two-kernel form behind (flag, 1)
        R, dx, dE = filled(B, ldr), filled(B, D), filled(B, T * D)
        fused_fwd(kind, x, ws, rows, bags, D, 0, R, pred=(flag, 0))
        if kind == "bf16":
            ops.interact_bwd_gather_narrow_bf16(x, ws, bags, D, 0, dR, dx, dE, pred=(flag, 0))
        E2 = pooled(kind, ws, rows, bags, B, D, pred=(flag, 1))
        R2, dx2, dE2 = filled(B, ldr), filled(B, D), filled(B, T * D)
        ops.interact_fwd((x, E_ref), D, 0, R2, pred=(flag, 1))
        ops.interact_bwd((x, E_ref), D, 0, dR, (dx2, dE2), pred=(flag, 1))
        ops.check_index_errors(sync=True)
        if fused_runs:
            assert same_bits(R, ref) and untouched(E2, R2, dx2, dE2)
            if kind == "bf16":
                assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
        else:
            assert untouched(R, dx, dE)
            assert same_bits(E2, E_ref) and same_bits(R2, ref) and same_bits(dx2, dx_ref) and same_bits(dE2, dE_ref)
    # ... and the opposite sense of both
    R = filled(B, ldr)
    fused_fwd(kind, x, ws, rows, bags, D, 0, R, pred=(one, 1))
    assert same_bits(R, ref)
    R = filled(B, ldr)
    fused_fwd(kind, x, ws, rows, bags, D, 0, R, pred=(zero, 1))
    assert untouched(R)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 7. refusals
def offset_view(t, nbytes):
    """the same table at `nbytes` past a fresh (256-byte aligned) allocation"""
    es = t.element_size()
    assert nbytes % es == 0
    raw = torch.empty(t.numel() + nbytes // es, dtype=t.dtype, device=t.device)
    v = raw[nbytes // es:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == nbytes
    return v


def test_refused_operands_bf16():
    from dlrm_amd import ops
    B, D = 8, 16
    w = torch.randn((10, D), device=dev()).to(torch.bfloat16)
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, D, 0)), device=dev())
    dR = dR_of(B, 2, D, 0)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, D), device=dev())
    ops.interact_fwd_gather_narrow_bf16(x, [w], bags, D, 0, R)                       # (the operands are fine as they stand)
    ops.interact_bwd_gather_narrow_bf16(x, [w], bags, D, 0, dR, dx, dE)
    assert ops.gather_narrow_bf16_ok(2, 16) and not ops.gather_narrow_bf16_ok(2, 128) and not ops.gather_narrow_bf16_ok(2, 48)
    for d in (128, 48):
        wd, xd = torch.zeros((10, d), device=dev(), dtype=torch.bfloat16), torch.zeros((B, d), device=dev())
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow_bf16(xd, [wd], bags, d, 0, torch.empty((B, d + 4), device=dev()))
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_bwd_gather_narrow_bf16(xd, [wd], bags, d, 0, torch.zeros((B, d + 4), device=dev()), torch.empty((B, d), device=dev()),
                                                torch.empty((B, d), device=dev()))
    # the D = 128 bf16 kernels keep refusing D = 16
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather(x, [w], bags, D, 0, R)
    # fp32 tables are not this call's
    with pytest.raises(RuntimeError):
        ops.interact_fwd_gather_narrow_bf16(x, [w.float()], bags, D, 0, R)
    # a table base that is not 8-byte aligned: views 2, 4 and 6 bytes in; 8 bytes in is fine (and gives the same bits)
    for nbytes in (2, 4, 6):
        odd = offset_view(w, nbytes)
        assert not ops.narrow_bf16_tables_aligned([odd])
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow_bf16(x, [odd], bags, D, 0, R)
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_bwd_gather_narrow_bf16(x, [odd], bags, D, 0, dR, dx, dE)
    R8 = torch.empty_like(R)
    ops.interact_fwd_gather_narrow_bf16(x, [offset_view(w, 8)], bags, D, 0, R8)
    assert same_bits(R8, R)
    # per-sample weights
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_fwd_gather_narrow_bf16(x, [w], wbags, D, 0, R)
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_bwd_gather_narrow_bf16(x, [w], wbags, D, 0, dR, dx, dE)
    # nnz != B
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_fwd_gather_narrow_bf16(x, [w], mbags, D, 0, R)
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_bwd_gather_narrow_bf16(x, [w], mbags, D, 0, dR, dx, dE)
    ops.check_index_errors(sync=True)


def test_refused_operands_quant():
    from dlrm_amd import ops
    B, D = 8, 16
    W = torch.randn((10, D), device=dev())
    q8, q4 = ops.emb_quantize(W, 8), ops.emb_quantize(W, 4)
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, D, 0)), device=dev())
    R4 = torch.empty_like(R)
    ops.interact_fwd_gather_narrow_quant(x, [q8], [10], D, 8, bags, 0, R)                       # (the operands are fine as they stand)
    ops.interact_fwd_gather_narrow_quant(x, [q4], [10], D, 4, bags, 0, R4)
    assert ops.gather_narrow_quant_ok(2, 16, 8) and ops.gather_narrow_quant_ok(32, 64, 4)
    assert not ops.gather_narrow_quant_ok(2, 128, 8) and not ops.gather_narrow_quant_ok(2, 48, 4) and not ops.gather_narrow_quant_ok(2, 16, 16)
    for d in (128, 48):
        qd = ops.emb_quantize(torch.randn((10, d), device=dev()), 8)
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow_quant(torch.zeros((B, d), device=dev()), [qd], [10], d, 8, bags, 0, torch.empty((B, d + 4), device=dev()))
    # the D = 128 kernel keeps refusing D = 16
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather_quant(x, [q8], [10], D, 8, bags, 0, R.clone())
    # bits = 16
    with pytest.raises(RuntimeError, match="4 or 8 bits"):
        ops.interact_fwd_gather_narrow_quant(x, [q8], [10], D, 16, bags, 0, R.clone())
    # unaligned packed tables: 8 bits needs 8 bytes, 4 bits needs 4
    for nbytes in (1, 2, 4):
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow_quant(x, [offset_view(q8, nbytes)], [10], D, 8, bags, 0, R.clone())
    for nbytes in (1, 2, 3):
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow_quant(x, [offset_view(q4, nbytes)], [10], D, 4, bags, 0, R.clone())
    Ra, Rb = torch.empty_like(R), torch.empty_like(R)
    ops.interact_fwd_gather_narrow_quant(x, [offset_view(q8, 8)], [10], D, 8, bags, 0, Ra)
    ops.interact_fwd_gather_narrow_quant(x, [offset_view(q4, 4)], [10], D, 4, bags, 0, Rb)
    assert same_bits(Ra, R) and same_bits(Rb, R4)
    # per-sample weights
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_fwd_gather_narrow_quant(x, [q8], [10], D, 8, wbags, 0, R.clone())
    # nnz != B
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_fwd_gather_narrow_quant(x, [q8], [10], D, 8, mbags, 0, R.clone())
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 8. the models
CRITEO_LIKE = [1460, 583, 2000, 1999, 305, 24, 1200, 633, 3, 931, 1500, 2000, 1890, 27, 1040, 1800, 10, 563, 201, 4, 2000, 18, 15, 1300, 105, 1420]
CONFIGS = {"d16_t26": (16, CRITEO_LIKE), "d64_t3": (64, CRITEO_LIKE[:3])}


def fp32_model(cfg, **kw):
    import dlrm_amd
    from dlrm_amd import ops
    d, ln_emb = CONFIGS[cfg]
    np.random.seed(3)
    torch.manual_seed(3)
    F = len(ln_emb) + 1
    interaction = kw.pop("interaction", "dot")
    n_top = d * F if interaction == "cat" else d + F * (F - 1) // 2
    m = dlrm_amd.DLRM_Net(d, np.asarray(ln_emb), np.asarray([13, 32, d]), np.asarray([n_top, 32, 1]), interaction,
                          sigmoid_top=1, loss_function="bce", **kw).to(dev())
    m.emb_update_mode = ops.UPD_SORTED
    return m


def bf16_model(cfg, narrow, bf16, rounding="nearest", seed=0):
    m = fp32_model(cfg)
    m.embedding_bfloat16(rounding, seed)
    m.fuse_narrow_interact, m.fuse_bf16_interact = narrow, bf16
    return m


def batch(cfg, seed, B, state="tagged", hots=1):
    from dlrm_amd import ops
    ln_emb = CONFIGS[cfg][1]
    rng = np.random.default_rng(seed)
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) * hots for _ in ln_emb]
    lS_i = [to_dev(rng.integers(0, n, size=B * hots).astype(np.int64)) for n in ln_emb]
    target = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    if state == "tagged":
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    if state == "ragged":
        lS_o[1][17] = 16                # bag 16 has two lookups, bag 17 none: nnz == B, not one lookup per bag
    return X, lS_o, lS_i, target


class Counted:
    """wraps the ops of both forms: which path did the model take"""

    def __init__(self, monkeypatch, names):
        from dlrm_amd import ops
        self.names = names
        self.n = {k: 0 for k in names}
        self.preds = {k: [] for k in names}
        for name in names:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, f0):
        def f(*a, **k):
            self.n[name] += 1
            self.preds[name].append(k.get("pred"))
            return f0(*a, **k)
        return f

    def counts(self):
        return tuple(self.n[k] for k in self.names)


BF16_NAMES = ("interact_fwd_gather_narrow_bf16", "interact_bwd_gather_narrow_bf16", "emb_fwd_bf16", "interact_fwd", "interact_bwd")
QUANT_NAMES = ("interact_fwd_gather_narrow_quant", "emb_fwd_quant", "interact_fwd")


def predict(m, X, lS_o, lS_i):
    from dlrm_amd import ops
    with torch.no_grad():
        Z = m(X, lS_o, lS_i)
    ops.check_index_errors(sync=True)
    return Z


def one_step(m, opt, X, lS_o, lS_i, target):
    opt.zero_grad()
    loss = m.loss_fn(m(X, lS_o, lS_i), target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach())


def same_state(a, b, oa=None, ob=None):
    for t, (ea, eb) in enumerate(zip(a.emb_l, b.emb_l)):
        assert ea.weight.dtype == torch.bfloat16 and eb.weight.dtype == torch.bfloat16
        assert np.array_equal(bits16(ea.weight), bits16(eb.weight)), "table %d" % t
        if oa is not None:
            sa, sb = oa.state[ea.weight]["momentum"], ob.state[eb.weight]["momentum"]
            assert same_bits(sa, sb), "accumulator %d" % t
    for tower in ("bot_l", "top_l"):
        for pa, pb in zip(getattr(a, tower).parameters(), getattr(b, tower).parameters()):
            assert same_bits(pa, pb), tower


@pytest.mark.parametrize("state", ["tagged", "fresh", "ragged"])
@pytest.mark.parametrize("optimizer", ["sgd_nearest", "sgd_stochastic", "adagrad"])
@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("cfg", ["d16_t26", "d64_t3"])
def test_bf16_model_gives_the_bits_of_the_two_kernel_form(cfg, B, optimizer, state, monkeypatch):
    """tagged: producer-tagged offsets -> the fused kernels alone.  fresh: offsets nobody vouched for -> the fused kernels behind (flag, 0), the
    two-kernel form behind (flag, 1), forward and backward.  ragged: nnz == B with an empty bag next to a two-lookup bag -> the results of
    the flags-off model.  Stochastic rounding: both models draw from the same seed, so the same dE gives the same rounded rows."""
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedRWSAdagrad, FusedSGD
    rounding = "stochastic" if optimizer == "sgd_stochastic" else "nearest"
    on, off = bf16_model(cfg, True, True, rounding, 9), bf16_model(cfg, False, False, rounding, 9)
    before = [bits16(e.weight).copy() for e in on.emb_l]

    def opt_of(m):
        return FusedRWSAdagrad(m.parameters(), lr=0.05) if optimizer == "adagrad" else FusedSGD(m.parameters(), lr=0.5)
    o_on, o_off = opt_of(on), opt_of(off)
    X, lS_o, lS_i, target = batch(cfg, 11 + B, B, state)
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, o_off, X, lS_o, lS_i, target)
    ops.check_index_errors(sync=True)
    if state != "tagged":
        lS_o = [o.clone() for o in lS_o]              # fresh tensor objects: no verdict is cached for them
    calls = Counted(monkeypatch, BF16_NAMES)
    got = predict(on, X, lS_o, lS_i)
    assert same_bits(got, want)
    if state == "tagged":
        assert calls.counts() == (1, 0, 0, 0, 0) and calls.preds["interact_fwd_gather_narrow_bf16"] == [None]
    else:
        assert calls.counts() == (1, 0, 1, 1, 0)
        assert calls.preds["interact_fwd_gather_narrow_bf16"][0][1] == 0 and calls.preds["emb_fwd_bf16"][0][1] == 1
        assert calls.preds["interact_fwd"][0][1] == 1
    if state != "tagged":
        lS_o = [o.clone() for o in lS_o]
    calls = Counted(monkeypatch, BF16_NAMES)
    l_on = one_step(on, o_on, X, lS_o, lS_i, target)
    ops.check_index_errors(sync=True)
    if state == "tagged":
        assert calls.counts() == (1, 1, 0, 0, 0)
    else:
        assert calls.counts() == (1, 1, 1, 1, 1)
        assert calls.preds["interact_bwd_gather_narrow_bf16"][0][1] == 0 and calls.preds["interact_bwd"][0][1] == 1
    assert l_on == l_off
    if optimizer == "adagrad":
        same_state(on, off, o_on, o_off)
    else:
        same_state(on, off)
    assert any(not np.array_equal(w0, bits16(e.weight)) for w0, e in zip(before, on.emb_l))       # (the step moved the tables)


@pytest.mark.parametrize("flags", [(True, False), (False, True), (False, False)])
def test_bf16_model_with_either_flag_off_never_calls_the_new_ops(flags, monkeypatch):
    from dlrm_amd.optim import FusedSGD
    m = bf16_model("d16_t26", *flags)
    X, lS_o, lS_i, target = batch("d16_t26", 5, 64)
    calls = Counted(monkeypatch, BF16_NAMES)
    predict(m, X, lS_o, lS_i)
    assert calls.counts() == (0, 0, 1, 1, 0)
    one_step(m, FusedSGD(m.parameters(), lr=0.5), X, lS_o, lS_i, target)
    assert calls.counts() == (0, 0, 2, 2, 1)


def quant_model(cfg, bits, **kw):
    m = fp32_model(cfg, **kw)
    m.quantize_embedding(bits)
    return m


def quant_forward(m, X, lS_o, lS_i, narrow, quant=True):
    from dlrm_amd import ops
    m.fuse_narrow_interact, m.fuse_quant_interact = narrow, quant
    with torch.no_grad():
        Z = m(X, lS_o, lS_i)
    ops.check_index_errors(sync=True)
    assert Z.grad_fn is None
    return Z


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("cfg", ["d16_t26", "d64_t3"])
def test_quant_model_flags_on_equal_off(cfg, B, bits, monkeypatch):
    from dlrm_amd import ops
    m = quant_model(cfg, bits)
    calls = Counted(monkeypatch, QUANT_NAMES)
    # tagged offsets: the fused kernel alone
    X, lS_o, lS_i, _ = batch(cfg, 11 + B, B)
    want = quant_forward(m, X, lS_o, lS_i, False)
    assert calls.counts() == (0, 1, 1)
    got = quant_forward(m, X, lS_o, lS_i, True)
    assert calls.counts() == (1, 1, 1) and calls.preds["interact_fwd_gather_narrow_quant"] == [None]
    assert same_bits(got, want)
    # fresh untagged offsets: fused behind (flag, 0), the two kernels behind (flag, 1)
    X, lS_o, lS_i, _ = batch(cfg, 12 + B, B, "fresh")
    want = quant_forward(m, X, lS_o, lS_i, False)
    lS_o = [o.clone() for o in lS_o]
    got = quant_forward(m, X, lS_o, lS_i, True)
    assert calls.counts() == (2, 3, 3) and calls.preds["interact_fwd_gather_narrow_quant"][-1][1] == 0
    assert calls.preds["emb_fwd_quant"][-1][1] == 1 and calls.preds["interact_fwd"][-1][1] == 1
    assert same_bits(got, want)
    # a ragged batch with nnz == B: flag path, the result is the two-kernel form's
    X, lS_o, lS_i, _ = batch(cfg, 13 + B, B, "ragged")
    want = quant_forward(m, X, lS_o, lS_i, False)
    lS_o = [o.clone() for o in lS_o]
    got = quant_forward(m, X, lS_o, lS_i, True)
    assert calls.n["interact_fwd_gather_narrow_quant"] == 3
    assert same_bits(got, want)
    # either flag off (and fuse_emb_interact off): the new op is not called
    quant_forward(m, X, lS_o, lS_i, True, quant=False)
    quant_forward(m, X, lS_o, lS_i, False, quant=True)
    m.fuse_emb_interact = False
    quant_forward(m, X, lS_o, lS_i, True)
    assert calls.n["interact_fwd_gather_narrow_quant"] == 3


@pytest.mark.parametrize("bits", [8, 4])
def test_evaluate_inference_takes_the_fused_form(bits, monkeypatch):
    from dlrm_amd import evaluate
    cfg = "d16_t26"
    m = quant_model(cfg, bits)
    rng = np.random.default_rng(31)
    batches = []
    for s in range(2):
        X, lS_o, lS_i, _ = batch(cfg, 32 + s, 150, "fresh")
        Tg = torch.from_numpy(np.round(rng.random((150, 1))).astype(np.float32))
        batches.append((X.cpu(), [o.cpu() for o in lS_o], [i.cpu() for i in lS_i], Tg))
    m.fuse_narrow_interact = False
    want = evaluate.inference(m, batches, device=dev())
    calls = Counted(monkeypatch, QUANT_NAMES)
    m.fuse_narrow_interact = True
    got = evaluate.inference(m, batches, device=dev())
    assert calls.n["interact_fwd_gather_narrow_quant"] == 2
    assert got == want


@pytest.mark.parametrize("case", ["multihot", "cat", "pooling_weights", "gradients"])
def test_other_quant_models_keep_the_two_kernel_form(case, monkeypatch):
    from dlrm_amd import ops
    cfg = "d16_t26"
    m = quant_model(cfg, 8, interaction="cat") if case == "cat" else quant_model(cfg, 8, weighted_pooling="fixed") \
        if case == "pooling_weights" else quant_model(cfg, 8)
    calls = Counted(monkeypatch, QUANT_NAMES)
    X, lS_o, lS_i, _ = batch(cfg, 41, 64, hots=3 if case == "multihot" else 1)
    if case == "gradients":                   # a forward that trains the bottom tower keeps InteractFunction's autograd node
        m.fuse_narrow_interact = m.fuse_quant_interact = True
        Z = m(X, lS_o, lS_i)
        ops.check_index_errors(sync=True)
        assert Z.grad_fn is not None and calls.n["interact_fwd_gather_narrow_quant"] == 0 and calls.n["emb_fwd_quant"] == 1
        return
    want = quant_forward(m, X, lS_o, lS_i, False)
    got = quant_forward(m, X, lS_o, lS_i, True)
    assert calls.n["interact_fwd_gather_narrow_quant"] == 0 and calls.n["emb_fwd_quant"] == 2
    assert same_bits(got, want)
