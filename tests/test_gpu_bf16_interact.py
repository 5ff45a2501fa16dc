"""Fused lookup + interaction over bfloat16 tables, forward and backward: dlrm_interact_fwd_gather_bf16 / dlrm_interact_bwd_gather_bf16 /
dlrm_emb_fwd_bf16_pred through dlrm_amd.ops (ops.interact_fwd_gather / ops.interact_bwd_gather dispatch on the tables' dtype), and
DLRM_Net.fuse_bf16_interact.

  * op level: R, dx, dE are BIT-IDENTICAL to the two-kernel form (ops.emb_fwd_bf16 into a feature buffer, then ops.interact_fwd /
    ops.interact_bwd over it) and, for in-range ids, to the fp32 fused kernels on the tables upcast to fp32; one test is independent of the
    project's kernels (float64 numpy from the bf16 bit patterns);
  * model level: fuse_bf16_interact = True gives the prediction bits, the loss and — after one optimizer step — the table bits, the
    Adagrad accumulators and the tower parameters of fuse_bf16_interact = False.
"""
import numpy as np
import pytest
import torch

import test_bf16_emb_host as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = 128
ROWS = [1, 37, 2000, 3, 513, 1200, 2, 64, 1999, 17, 300, 5, 1024, 77, 2000, 9, 450, 31, 1500, 4, 800, 129, 11, 1777, 256, 60]      # 26 tables


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def bf16_table(h):
    """uint16 bit patterns [rows, D] -> torch.bfloat16 GPU tensor"""
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16)).to(dev()).view(torch.bfloat16)


def bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


SPECIAL = np.array([0x8000, 0x0001, 0x8001, 0x007F, 0x0040, 0x807F, 0x0000, 0x0080], dtype=np.uint16)   # -0.0, bf16 subnormals (both signs), +0.0, the smallest normal

_tables = {}


def tables(T):
    """(bf16 tables, their fp32 upcasts) of ROWS[t] rows, uniform in [-1, 1] rounded to bf16.  The single row of table 0 carries -0.0 and
    bf16 subnormals in its first columns, the first ten rows of table 1 consist of them."""
    if "all" not in _tables:
        rng = np.random.default_rng(2024)
        ws = []
        for t, n in enumerate(ROWS):
            h = H.round_nearest(rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32))
            if t == 0:
                h[0, :SPECIAL.size] = SPECIAL
            if t == 1:
                h[:10] = np.tile(SPECIAL, D // SPECIAL.size)[None, :]
            ws.append(bf16_table(h))
        _tables["all"] = (ws, [w.float() for w in ws])
    ws, up = _tables["all"]
    return ws[:T], up[:T]


def onehot_bags(rng, rows, B, idx_dtype=torch.int64):
    from dlrm_amd import ops
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    return ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows], [to_dev(i, idx_dtype) for i in idx]), idx


def ldr_of(F, mode):
    from dlrm_amd import ops
    return (ops.interact_out_width(F, D, mode) + 3) & ~3


def guarded(B, ld):
    """[B, ld] view in the middle of a NaN-filled [B + 2, ld] allocation: rows -1 and B are the canaries"""
    buf = torch.full((B + 2, ld), float("nan"), device=dev())
    return buf, buf[1:B + 1]


def canaries_intact(*bufs):
    return all(bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[-1]).all()) for b in bufs)


def pooled(ws, bags, B):
    """the [B, T*D] fp32 buffer of the two-kernel form"""
    from dlrm_amd import ops
    E = torch.empty((B, len(ws) * D), device=dev())
    ops.emb_fwd_bf16(ws, bags, E)
    return E


def x_with_zeros_and_negatives(B, g=None):
    x = torch.randn((B, D), device=dev(), generator=g)
    x[:, 5::16] = 0.0
    return x


def dR_of(B, F, mode, g=None):
    from dlrm_amd import ops
    Wd = ops.interact_out_width(F, D, mode)
    dR = torch.zeros((B, ldr_of(F, mode)), device=dev())
    dR[:, :Wd] = torch.randn((B, Wd), device=dev(), generator=g)
    return dR


# ------------------------------------------------------------------------------------------------ 1. the forward grid
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_forward_bit_identity_grid(F, idx_dtype):
    """B = 1 / 3 / 5 leave waves and workgroups without a sample; B = 5000 exceeds twice the samples one pass of the grid covers (256
    workgroups x 4 at F > 16, 512 x 4 at F <= 16): some waves run the prologue, a steady-state iteration and the clamped tail, others one
    iteration fewer.  F = 16 / 17 straddle the NB = 1 / 2 instantiations."""
    from dlrm_amd import ops
    T = F - 1
    ws, up = tables(T)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000, 5000):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = torch.randn((B, D), device=dev())
        E = pooled(ws, bags, B)
        for mode in (0, 1, 2):
            ldr = ldr_of(F, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref = torch.empty((B, ldr), device=dev())
            ops.interact_fwd((x, E), D, mode, ref)
            ref32 = torch.empty((B, ldr), device=dev())
            ops.interact_fwd_gather(x, up, bags, D, mode, ref32)
            buf1, R1 = guarded(B, ldr)
            buf2, R2 = guarded(B, ldr)
            ops.interact_fwd_gather(x, ws, bags, D, mode, R1)
            ops.interact_fwd_gather(x, ws, bags, D, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert same_bits(R1, ref), what + ": the two-kernel form"
            assert same_bits(R1, ref32), what + ": the fp32 fused kernel on the upcast tables"
            assert same_bits(R1, R2), what + ": two runs differ"
            assert canaries_intact(buf1, buf2), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. the backward grid
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_backward_bit_identity_grid(F, idx_dtype):
    from dlrm_amd import ops
    T = F - 1
    ws, up = tables(T)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10 + 1)
    ops.check_index_errors(sync=True)
    for B in (1, 5, 64, 5000):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = x_with_zeros_and_negatives(B)
        assert bool((x == 0).any()) and bool((x < 0).any())
        E = pooled(ws, bags, B)
        for mode in (0, 1, 2):
            dR = dR_of(B, F, mode)
            for relu in (0, ops.INTERACT_RELU_X):
                m = mode | relu
                dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
                ops.interact_bwd((x, E), D, m, dR, (dx_ref, dE_ref))
                dx32, dE32 = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
                ops.interact_bwd_gather(x, up, bags, D, m, dR, dx32, dE32)
                outs = []
                for _ in range(2):
                    bx, dx = guarded(B, D)
                    be, dE = guarded(B, T * D)
                    ops.interact_bwd_gather(x, ws, bags, D, m, dR, dx, dE)
                    outs.append((bx, dx, be, dE))
                ops.check_index_errors(sync=True)
                (bx, dx, be, dE), (bx2, dx2, be2, dE2) = outs
                what = "B=%d mode=%d relu=%d" % (B, mode, relu)
                assert not torch.isnan(dx).any() and not torch.isnan(dE).any(), what
                assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref), what + ": the two-kernel form"
                assert same_bits(dx, dx32) and same_bits(dE, dE32), what + ": the fp32 fused kernel on the upcast tables"
                assert same_bits(dx, dx2) and same_bits(dE, dE2), what + ": two runs differ"
                assert canaries_intact(bx, be, bx2, be2), what
                if relu:
                    assert bool((dx[x <= 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------ 3. independent of the project's kernels
def test_against_float64_numpy():
    """R, dx, dE against oracle.interact_fwd / oracle.interact_bwd (float64) on rows gathered in numpy from the upcast bit patterns, at the
    bar of tests/test_gpu_kernels.py::test_interact_fwd_bwd for B <= 67: forward rtol 1e-5, atol 1e-5; backward rtol 1e-5, atol 2e-5.
    The 0.25 scale of the table values is the one of tests/test_gpu_quant_interact.py::test_against_float64_numpy, for its reason: with
    unit-variance operands on both sides the worst of ~22 k fp32 128-term dots lies ABOVE that bar whatever the kernel; with tables drawn
    N(0, 0.25^2) beside x ~ N(0, 1) the round-off is 1/16 (table pairs) or 1/4 (x pairs) of that, while one wrong bf16 element
    (2^-8 relative) still moves an output by many times the bar."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows = ROWS[:T]
    rng = np.random.default_rng(303)
    hs = [H.round_nearest((0.25 * rng.standard_normal((n, D))).astype(np.float32)) for n in rows]
    ws = [bf16_table(h) for h in hs]
    bags, idx = onehot_bags(np.random.default_rng(33), rows, B)
    x = to_dev(rng.standard_normal((B, D)).astype(np.float32))
    Wd = ops.interact_out_width(F, D, 0)
    ldr = ldr_of(F, 0)
    dRn = rng.standard_normal((B, Wd)).astype(np.float32)
    dR = torch.zeros((B, ldr), device=dev())
    dR[:, :Wd] = to_dev(dRn)
    R = torch.empty((B, ldr), device=dev())
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_fwd_gather(x, ws, bags, D, 0, R)
    ops.interact_bwd_gather(x, ws, bags, D, 0, dR, dx, dE)
    ops.check_index_errors(sync=True)
    feat = np.empty((B, F, D), dtype=np.float32)
    feat[:, 0] = x.cpu().numpy()
    for t in range(T):
        feat[:, 1 + t] = H.bf16_to_f32(hs[t])[idx[t]]
    want = O.interact_fwd(feat, False)
    dwant = O.interact_bwd(feat, dRn, False)
    got = R.cpu().numpy()

    def ratio(g, w, atol):
        return float((np.abs(g - w) / (atol + 1e-5 * np.abs(w))).max())
    gx, gE = dx.cpu().numpy(), dE.cpu().numpy().reshape(B, T, D)
    print("worst error / (atol + rtol |want|): forward %.3g, dx %.3g, dE %.3g"
          % (ratio(got[:, :Wd], want, 1e-5), ratio(gx, dwant[:, 0], 2e-5), ratio(gE, dwant[:, 1:], 2e-5)))
    np.testing.assert_allclose(got[:, :Wd], want, rtol=1e-5, atol=1e-5)
    assert (got[:, Wd:] == 0).all()
    np.testing.assert_allclose(gx, dwant[:, 0], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(gE, dwant[:, 1:], rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 4. rows beyond 4 GiB
def test_rows_beyond_4_gib():
    """one bf16 table of 17 M rows (4.35 GB, never filled as a whole): only the rows the lookups name are written, from a small table"""
    import test_gpu_bigtables as BT
    from dlrm_amd import ops
    BIG, B = 17_000_000, 1000
    rng = np.random.default_rng(44)
    ids = BT.high_indices(rng, BIG, B)                         # top eighth, plus row 0 and the last row
    assert int(ids.max()) * 256 > 2 ** 32 and ids.min() == 0 and ids.max() == BIG - 1
    small = bf16_table(H.round_nearest(rng.uniform(-1.0, 1.0, size=(B, D)).astype(np.float32)))
    big = torch.empty((BIG, D), dtype=torch.bfloat16, device=dev())
    uniq = np.unique(ids)
    big.index_copy_(0, to_dev(uniq), small[:uniq.size])
    try:
        for idx_dtype in (torch.int64, torch.int32):
            bags = ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype)], [to_dev(ids, idx_dtype)])
            x = x_with_zeros_and_negatives(B)
            ldr = ldr_of(2, 0)
            E = pooled([big], bags, B)
            assert same_bits(E, small[:uniq.size].float()[to_dev(np.searchsorted(uniq, ids))] + 0.0)      # the rows really are the small table's
            ref, R = torch.empty((B, ldr), device=dev()), torch.full((B, ldr), float("nan"), device=dev())
            ops.interact_fwd((x, E), D, 0, ref)
            ops.interact_fwd_gather(x, [big], bags, D, 0, R)
            dR = dR_of(B, 2, 0)
            dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, D), device=dev())
            ops.interact_bwd((x, E), D, 0, dR, (dx_ref, dE_ref))
            dx, dE = torch.full((B, D), float("nan"), device=dev()), torch.full((B, D), float("nan"), device=dev())
            ops.interact_bwd_gather(x, [big], bags, D, 0, dR, dx, dE)
            ops.check_index_errors(sync=True)
            assert same_bits(R, ref)
            assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5. bad input
def test_out_of_range_ids_are_reported_and_give_the_zero_row():
    from dlrm_amd import ops
    B, F = 50, 4
    ws, _ = tables(3)
    rows = ROWS[:3]
    rng = np.random.default_rng(5)
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    idx[1][7] = rows[1] + 3            # too large
    idx[2][31] = -1                    # negative
    offs = [torch.arange(B, device=dev()) for _ in rows]

    def bags():
        return ops.BagBatch(offs, [to_dev(i) for i in idx])
    x = x_with_zeros_and_negatives(B)
    ldr = ldr_of(F, 0)
    dR = dR_of(B, F, 0)
    ops.check_index_errors(sync=True)
    # the two-kernel form: its lookup reports the same ids
    E = pooled(ws, bags(), B)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd((x, E), D, 0, dR, (dx_ref, dE_ref))
    ops.check_index_errors(sync=True)
    # forward
    R = torch.full((B, ldr), float("nan"), device=dev())
    ops.interact_fwd_gather(x, ws, bags(), D, 0, R)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(R, ref)
    # pairs (2, 0) and (3, 0) of the bad samples: x . zero row = +0.0
    zero_bits = R[[7, 31], [D + 1, D + 3]].view(torch.int32)
    assert bool((zero_bits == 0).all())
    ops.check_index_errors(sync=True)            # reported once
    # backward: the gradient row of the bad lookup is written like any other
    dx, dE = torch.full((B, D), float("nan"), device=dev()), torch.full((B, 3 * D), float("nan"), device=dev())
    ops.interact_bwd_gather(x, ws, bags(), D, 0, dR, dx, dE)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
    ops.check_index_errors(sync=True)


def test_broken_bag_start_is_reported():
    from dlrm_amd import ops
    B = 40
    ws, _ = tables(2)
    rows = ROWS[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    bags = ops.BagBatch([torch.arange(B, device=dev()), to_dev(off)], [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows])
    x = torch.randn((B, D), device=dev())
    R = torch.empty((B, ldr_of(3, 0)), device=dev())
    ops.check_index_errors(sync=True)
    ops.interact_fwd_gather(x, ws, bags, D, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, 2 * D), device=dev())
    ops.interact_bwd_gather(x, ws, bags, D, 0, dR_of(B, 3, 0), dx, dE)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 6. predicates
def test_launch_predicates():
    from dlrm_amd import ops
    B, F = 70, 5
    T = F - 1
    ws, _ = tables(T)
    bags, _ = onehot_bags(np.random.default_rng(8), ROWS[:T], B)
    x = x_with_zeros_and_negatives(B)
    ldr = ldr_of(F, 0)
    dR = dR_of(B, F, 0)
    E_ref = pooled(ws, bags, B)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_ref), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E_ref), D, 0, dR, (dx_ref, dE_ref))
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())
    for flag, nonzero, runs in ((zero, 0, True), (one, 1, True), (zero, 1, False), (one, 0, False)):
        nan = float("nan")
        R = torch.full((B, ldr), nan, device=dev())
        E = torch.full((B, T * D), nan, device=dev())
        dx, dE = torch.full((B, D), nan, device=dev()), torch.full((B, T * D), nan, device=dev())
        ops.interact_fwd_gather(x, ws, bags, D, 0, R, pred=(flag, nonzero))
        ops.interact_bwd_gather(x, ws, bags, D, 0, dR, dx, dE, pred=(flag, nonzero))
        ops.emb_fwd_bf16(ws, bags, E, pred=(flag, nonzero))
        ops.check_index_errors(sync=True)
        if runs:
            assert same_bits(R, ref) and same_bits(E, E_ref) and same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
        else:
            assert all(bool(torch.isnan(t).all()) for t in (R, E, dx, dE))


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_operands():
    from dlrm_amd import ops
    B = 8
    assert ops.gather_bf16_ok(27, 128) and ops.gather_bf16_ok(2, 128)
    assert not ops.gather_bf16_ok(27, 64) and not ops.gather_bf16_ok(28, 128)
    w = bf16_table(H.round_nearest(np.random.default_rng(1).uniform(-1, 1, size=(10, D)).astype(np.float32)))
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, 0)), device=dev())
    dR = dR_of(B, 2, 0)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, D), device=dev())
    ops.interact_fwd_gather(x, [w], bags, D, 0, R)                       # (the operands are fine as they stand)
    ops.interact_bwd_gather(x, [w], bags, D, 0, dR, dx, dE)
    # D = 64
    w64 = torch.zeros((10, 64), dtype=torch.bfloat16, device=dev())
    x64 = x[:, :64].contiguous()
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather(x64, [w64], bags, 64, 0, torch.empty((B, 68), device=dev()))
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather(x64, [w64], bags, 64, 0, torch.zeros((B, 68), device=dev()), torch.empty((B, 64), device=dev()),
                                torch.empty((B, 64), device=dev()))
    # an unaligned table: a view at a 2-byte offset
    raw = torch.empty(10 * D + 1, dtype=torch.bfloat16, device=dev())
    odd = raw[1:].view(10, D)
    odd.copy_(w)
    assert odd.data_ptr() % 16 == 2 and not ops.bf16_tables_aligned([odd]) and ops.bf16_tables_aligned([w])
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather(x, [odd], bags, D, 0, R)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather(x, [odd], bags, D, 0, dR, dx, dE)
    # mixed dtypes
    bags2 = ops.BagBatch([torch.arange(B, device=dev())] * 2, [torch.zeros(B, dtype=torch.int64, device=dev())] * 2)
    R3 = torch.empty((B, ldr_of(3, 0)), device=dev())
    with pytest.raises(RuntimeError, match="ONE dtype"):
        ops.interact_fwd_gather(x, [w, w.float()], bags2, D, 0, R3)
    with pytest.raises(RuntimeError, match="ONE dtype"):
        ops.interact_bwd_gather(x, [w.float(), w], bags2, D, 0, dR_of(B, 3, 0), dx, torch.empty((B, 2 * D), device=dev()))
    # per-sample weights
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_fwd_gather(x, [w], wbags, D, 0, R)
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_bwd_gather(x, [w], wbags, D, 0, dR, dx, dE)
    # nnz != B
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_fwd_gather(x, [w], mbags, D, 0, R)
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_bwd_gather(x, [w], mbags, D, 0, dR, dx, dE)
    # the update inside the backward exists for fp32 tables only
    with pytest.raises(RuntimeError, match="presorted"):
        ops.interact_bwd_gather(x, [w], bags, D, 0, dR, dx, dE, presorted=object())
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 8. the model
CRITEO_LIKE = [1460, 583, 2000, 1999, 305, 24, 1200, 633, 3, 931, 1500, 2000, 1890, 27, 1040, 1800, 10, 563, 201, 4, 2000, 18, 15, 1300, 105, 1420]


def fp32_model(d=D, **kw):
    import dlrm_amd
    np.random.seed(3)
    torch.manual_seed(3)
    T = len(CRITEO_LIKE)
    F = T + 1
    interaction = kw.pop("interaction", "dot")
    n_top = d * F if interaction == "cat" else d + F * (F - 1) // 2
    return dlrm_amd.DLRM_Net(d, np.asarray(CRITEO_LIKE), np.asarray([13, 64, d]), np.asarray([n_top, 64, 1]), interaction,
                             sigmoid_top=1, loss_function="bce", **kw).to(dev())


def bf16_model(fused, rounding="nearest", seed=0, d=D, **kw):
    """identically built bf16 models (as build_pair of tests/test_gpu_bf16_emb.py): same seeds, converted after construction"""
    m = fp32_model(d, **kw)
    m.embedding_bfloat16(rounding, seed)
    m.fuse_bf16_interact = fused
    return m


def batch(seed, B=200, hots=1, tagged=True):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) * hots for _ in CRITEO_LIKE]
    lS_i = [to_dev(rng.integers(0, n, size=B * hots).astype(np.int64)) for n in CRITEO_LIKE]
    target = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    if tagged:
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    return X, lS_o, lS_i, target


class Counted:
    """wraps ops.interact_fwd_gather / ops.interact_bwd_gather / ops.emb_fwd_bf16: which path did the model take"""

    def __init__(self, monkeypatch):
        from dlrm_amd import ops
        self.fwd, self.bwd, self.lookup, self.preds = 0, 0, 0, []
        f0, b0, l0 = ops.interact_fwd_gather, ops.interact_bwd_gather, ops.emb_fwd_bf16

        def fwd(*a, **k):
            self.fwd += 1
            self.preds.append(k.get("pred"))
            return f0(*a, **k)

        def bwd(*a, **k):
            self.bwd += 1
            return b0(*a, **k)

        def lookup(*a, **k):
            self.lookup += 1
            return l0(*a, **k)
        monkeypatch.setattr(ops, "interact_fwd_gather", fwd)
        monkeypatch.setattr(ops, "interact_bwd_gather", bwd)
        monkeypatch.setattr(ops, "emb_fwd_bf16", lookup)


def predict(model, X, lS_o, lS_i):
    from dlrm_amd import ops
    with torch.no_grad():
        Z = model(X, lS_o, lS_i)
    ops.check_index_errors(sync=True)
    return Z


def one_step(model, opt, X, lS_o, lS_i, target):
    from dlrm_amd import ops
    opt.zero_grad()
    loss = model.loss_fn(model(X, lS_o, lS_i), target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    return float(loss.detach())


def same_tables_and_towers(a, b):
    assert all(e.weight.dtype == torch.bfloat16 for e in a.emb_l)
    for t, (ea, eb) in enumerate(zip(a.emb_l, b.emb_l)):
        assert np.array_equal(bits_of(ea.weight), bits_of(eb.weight)), "table %d" % t
    for tower in ("bot_l", "top_l"):
        for pa, pb in zip(getattr(a, tower).parameters(), getattr(b, tower).parameters()):
            assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), tower


def test_model_takes_the_fused_kernels_and_predicts_the_same_bits():
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedSGD
    on, off = bf16_model(True), bf16_model(False)
    a = fp32_model()
    a.load_state_dict({k: v.float() for k, v in off.state_dict().items()})
    X, lS_o, lS_i, target = batch(11)
    want = predict(off, X, lS_o, lS_i)
    saved = ops.timers
    try:
        ops.timers = ops.KernelTimers()
        got = predict(on, X, lS_o, lS_i)
        one_step(on, FusedSGD(on.parameters(), lr=0.5), X, lS_o, lS_i, target)
        cats = set(ops.timers.summary())
    finally:
        ops.timers = saved
    assert "emb_interact_fwd_bf16" in cats and "emb_interact_bwd_bf16" in cats, cats
    assert "emb_fwd_bf16" not in cats and "interact_fwd" not in cats and "interact_bwd" not in cats, cats
    assert same_bits(got, want)
    assert same_bits(got, predict(a, X, lS_o, lS_i))


@pytest.mark.parametrize("rounding,seed", [("nearest", 0), ("stochastic", 2024)])
def test_one_sgd_step_gives_the_bits_of_the_two_kernel_form(rounding, seed, monkeypatch):
    from dlrm_amd.optim import FusedSGD
    on, off = bf16_model(True, rounding, seed), bf16_model(False, rounding, seed)
    before = [bits_of(e.weight) for e in on.emb_l]
    X, lS_o, lS_i, target = batch(12)
    l_off = one_step(off, FusedSGD(off.parameters(), lr=0.5), X, lS_o, lS_i, target)
    calls = Counted(monkeypatch)
    l_on = one_step(on, FusedSGD(on.parameters(), lr=0.5), X, lS_o, lS_i, target)
    assert (calls.fwd, calls.bwd, calls.lookup) == (1, 1, 0) and calls.preds == [None]
    assert l_on == l_off
    same_tables_and_towers(on, off)
    assert any(not np.array_equal(x, bits_of(e.weight)) for x, e in zip(before, on.emb_l))       # (the step moved the tables)


def test_one_rowwise_adagrad_step_gives_the_bits_of_the_two_kernel_form():
    from dlrm_amd.optim import FusedRWSAdagrad
    on, off = bf16_model(True), bf16_model(False)
    X, lS_o, lS_i, target = batch(13)
    o_on, o_off = FusedRWSAdagrad(on.parameters(), lr=0.05), FusedRWSAdagrad(off.parameters(), lr=0.05)
    assert one_step(on, o_on, X, lS_o, lS_i, target) == one_step(off, o_off, X, lS_o, lS_i, target)
    for ea, eb in zip(on.emb_l, off.emb_l):
        sa, sb = o_on.state[ea.weight]["momentum"], o_off.state[eb.weight]["momentum"]
        assert sa.dtype == torch.float32 and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    same_tables_and_towers(on, off)


@pytest.mark.parametrize("case", ["untagged", "ragged", "fuse_emb_interact_off"])
def test_other_offsets_states_give_the_bits_of_the_two_kernel_form(case, monkeypatch):
    """untagged: fresh offsets nobody vouched for -> the device-flag path: the fused kernels behind (flag, 0), the two-kernel form behind
    (flag, 1), forward and backward.  ragged: nnz == B with an empty bag next to a two-lookup bag -> the flag path runs the two-kernel
    form.  fuse_emb_interact off: the fused branch is not entered."""
    from dlrm_amd.optim import FusedSGD
    on, off = bf16_model(True), bf16_model(False)
    X, lS_o, lS_i, target = batch(14, tagged=False)
    if case == "ragged":
        lS_o[4][17] = 16
    if case == "fuse_emb_interact_off":
        on.fuse_emb_interact = False
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, FusedSGD(off.parameters(), lr=0.5), X, lS_o, lS_i, target)
    lS_o = [o.clone() for o in lS_o]                  # fresh tensor objects: no verdict is cached for them
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert same_bits(got, want)
    if case == "fuse_emb_interact_off":
        assert (calls.fwd, calls.lookup) == (0, 1)
    else:
        assert calls.fwd == 1 and calls.lookup == 1 and calls.preds[-1] is not None and calls.preds[-1][1] == 0
    lS_o = [o.clone() for o in lS_o]
    l_on = one_step(on, FusedSGD(on.parameters(), lr=0.5), X, lS_o, lS_i, target)
    assert l_on == l_off
    same_tables_and_towers(on, off)


def test_evaluate_inference_takes_the_fused_forward(monkeypatch):
    from dlrm_amd import evaluate
    on, off = bf16_model(True), bf16_model(False)
    batches = []
    for s in range(2):
        X, lS_o, lS_i, Tg = batch(32 + s, B=150, tagged=False)
        batches.append((X.cpu(), [o.cpu() for o in lS_o], [i.cpu() for i in lS_i], Tg.cpu()))
    want = evaluate.inference(off, batches, device=dev())
    calls = Counted(monkeypatch)
    got = evaluate.inference(on, batches, device=dev())
    assert calls.fwd == 2
    assert got == want


@pytest.mark.parametrize("case", ["multihot", "cat", "pooling_weights", "d16"])
def test_other_models_keep_the_two_kernel_form(case, monkeypatch):
    kw = {"interaction": "cat"} if case == "cat" else {"weighted_pooling": "fixed"} if case == "pooling_weights" else {}
    d = 16 if case == "d16" else D
    on, off = bf16_model(True, d=d, **kw), bf16_model(False, d=d, **kw)
    X, lS_o, lS_i, _ = batch(41, hots=3 if case == "multihot" else 1, tagged=(case != "multihot"))
    want = predict(off, X, lS_o, lS_i)
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert (calls.fwd, calls.lookup) == (0, 1)
    assert same_bits(got, want)


def test_update_in_backward_keeps_the_step_time_update(monkeypatch):
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedSGD
    on, off = bf16_model(True), bf16_model(False)
    on.update_in_backward = True
    presorts = []
    p0 = ops.emb_presort
    monkeypatch.setattr(ops, "emb_presort", lambda *a, **k: presorts.append(1) or p0(*a, **k))
    o_on, o_off = FusedSGD(on.parameters(), lr=0.5), FusedSGD(off.parameters(), lr=0.5)
    for s in range(2):                                 # (the optimizer is bound at the first step: the second backward could update)
        X, lS_o, lS_i, target = batch(50 + s)
        assert one_step(on, o_on, X, lS_o, lS_i, target) == one_step(off, o_off, X, lS_o, lS_i, target)
    assert not presorts
    same_tables_and_towers(on, off)
