"""Fused lookup + interaction over plain fp32 tables of D = 16 / 32 / 64, forward and backward: dlrm_interact_fwd_gather_narrow /
dlrm_interact_bwd_gather_narrow through dlrm_amd.ops, the predicated two-kernel form at these widths (dlrm_emb_fwd_pred, dlrm_interact_fwd_pred /
dlrm_interact_bwd_pred without gather), and DLRM_Net.fuse_narrow_interact.

  * op level: R, dx, dE are BIT-IDENTICAL to the two-kernel form (ops.emb_fwd into a feature buffer, then ops.interact_fwd / ops.interact_bwd
    over it); one test is independent of the project's kernels (float64 numpy, any-order fp32 summation bounds);
  * model level: fuse_narrow_interact = True gives the prediction bits, the loss and — after one optimizer step — the table bits, the
    Adagrad accumulators and the tower parameters of fuse_narrow_interact = False; a captured step never runs the narrow kernels.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 37, 2000, 3, 513, 1200, 2, 64, 1999, 17, 300, 5, 1024, 77, 2000, 9, 450, 31, 1500, 4, 800, 129, 11, 1777, 256, 60]      # 26 tables
# one pass of a launch's grid covers gather_grid() x 4 samples (csrc/gather_common.h): 4 waves per workgroup, one sample per wave, and at
# most 256 CUs x 2 workgroups = 512 workgroups (256 x 1 where a workgroup's LDS exceeds 80 KiB) -> at most 2048 samples.  Twice that is 4096.
B_BIG = 4101
# -0.0, fp32 subnormals of both signs, +0.0, the smallest normal
SPECIAL = np.array([0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x807FFFFF, 0x00000000, 0x00800000], dtype=np.uint32).view(np.float32)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_tables = {}


def tables(T, D):
    """fp32 tables of ROWS[t] rows, uniform in [-1, 1].  The single row of table 0 carries -0.0 and fp32 subnormals in its first columns, the
    first ten rows of table 1 consist of them."""
    if D not in _tables:
        rng = np.random.default_rng(2024 + D)
        ws = []
        for t, n in enumerate(ROWS):
            h = rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32)
            if t == 0:
                h[0, :SPECIAL.size] = SPECIAL
            if t == 1:
                h[:10] = np.tile(SPECIAL, D // SPECIAL.size)[None, :]
            ws.append(to_dev(h))
        _tables[D] = ws
    return _tables[D][:T]


def onehot_bags(rng, rows, B, idx_dtype=torch.int64):
    from dlrm_amd import ops
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    return ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows], [to_dev(i, idx_dtype) for i in idx]), idx


def ldr_of(F, D, mode):
    from dlrm_amd import ops
    return (ops.interact_out_width(F, D, mode) + 3) & ~3


def guarded(B, w):
    """[B, w] column view (row pitch w + 8) in the middle of a NaN-filled [B + 2, w + 8] allocation: rows -1 and B and four columns on either
    side are the canaries"""
    buf = torch.full((B + 2, w + 8), float("nan"), device=dev())
    return buf, buf[1:B + 1, 4:4 + w]


def guarded_rows(B, ld):
    """[B, ld] view in the middle of a NaN-filled [B + 2, ld] allocation: rows -1 and B are the canaries (an R row is ldr wide: the kernels
    zero-fill up to the pitch, so R has no spare columns)"""
    buf = torch.full((B + 2, ld), float("nan"), device=dev())
    return buf, buf[1:B + 1]


def row_canaries_intact(*bufs):
    return all(bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[-1]).all()) for b in bufs)


def canaries_intact(*bufs):
    for b in bufs:
        if not (bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[-1]).all()) and bool(torch.isnan(b[:, :4]).all())
                and bool(torch.isnan(b[:, -4:]).all())):
            return False
    return True


def wide(t):
    """the same values as a column view of a wider allocation (ld = width + 8, still 16-byte aligned)"""
    buf = torch.full((t.size(0), t.size(1) + 8), 123.0, device=t.device)
    v = buf[:, 4:4 + t.size(1)]
    v.copy_(t)
    return v


def pooled(ws, bags, B, D):
    """the [B, T*D] fp32 buffer of the two-kernel form"""
    from dlrm_amd import ops
    E = torch.empty((B, len(ws) * D), device=dev())
    ops.emb_fwd(ws, bags, E)
    return E


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
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_forward_bit_identity_grid(D, F, idx_dtype):
    """B = 1 / 3 / 5 leave waves and workgroups without a sample; B_BIG = 4101 exceeds twice the samples one pass of the grid covers (see
    B_BIG): some waves run the prologue, a steady-state iteration and the clamped tail, others one iteration fewer.  F = 16 / 17 straddle
    the NB = 1 / 2 instantiations."""
    from dlrm_amd import ops
    T = F - 1
    ws = tables(T, D)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10 + D)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000, B_BIG):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = torch.randn((B, D), device=dev())
        E = pooled(ws, bags, B, D)
        for mode in (0, 1, 2):
            ldr = ldr_of(F, D, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref = torch.empty((B, ldr), device=dev())
            ops.interact_fwd((x, E), D, mode, ref)
            buf1, R1 = guarded_rows(B, ldr)
            buf2, R2 = guarded_rows(B, ldr)
            ops.interact_fwd_gather_narrow(x, ws, bags, D, mode, R1)
            ops.interact_fwd_gather_narrow(x, ws, bags, D, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert same_bits(R1, ref), what + ": the two-kernel form"
            assert same_bits(R1, R2), what + ": two runs differ"
            assert row_canaries_intact(buf1, buf2), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. the backward grid
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_backward_bit_identity_grid(D, F, idx_dtype):
    """the axes of the forward grid; x, dR, dx, dE are column views of wider allocations (ld = width + 8)"""
    from dlrm_amd import ops
    T = F - 1
    ws = tables(T, D)
    rows = ROWS[:T]
    rng = np.random.default_rng(F * 10 + D + 1)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000, B_BIG):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = wide(x_with_zeros_and_negatives(B, D))
        assert x.stride(0) == D + 8
        if B >= 5:
            assert bool((x == 0).any()) and bool((x < 0).any())
        E = pooled(ws, bags, B, D)
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
                    ops.interact_bwd_gather_narrow(x, ws, bags, D, m, dR, dx, dE)
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
def test_against_float64_numpy(D):
    """R, dx, dE against float64 numpy on rows gathered in numpy, within the any-order fp32 summation bounds (u = 2^-24):
    forward pair (a, b): |err| <= (D + 1) u sum_k |a_k| |b_k|;  backward: |err| <= (F + 2) u (sum_j |S_ij| |T_jd| + |dR_d|), the dR_d term for
    feature 0 only (the other rows have no such addend).  dR is random: S_ij differs for every pair, so a transposed or misplaced S entry
    moves the result by many times the bound."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows = ROWS[:T]
    rng = np.random.default_rng(303 + D)
    hs = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    ws = [to_dev(h) for h in hs]
    bags, idx = onehot_bags(np.random.default_rng(33), rows, B)
    xn = rng.standard_normal((B, D)).astype(np.float32)
    x = to_dev(xn)
    Wd = ops.interact_out_width(F, D, 0)
    ldr = ldr_of(F, D, 0)
    dRn = rng.standard_normal((B, Wd)).astype(np.float32)
    dR = torch.zeros((B, ldr), device=dev())
    dR[:, :Wd] = to_dev(dRn)
    R = torch.empty((B, ldr), device=dev())
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_fwd_gather_narrow(x, ws, bags, D, 0, R)
    ops.interact_bwd_gather_narrow(x, ws, bags, D, 0, dR, dx, dE)
    ops.check_index_errors(sync=True)
    feat = np.empty((B, F, D), dtype=np.float64)
    feat[:, 0] = xn
    for t in range(T):
        feat[:, 1 + t] = hs[t][idx[t]]
    u = 2.0 ** -24
    li, lj = np.tril_indices(F, -1)                   # row-major over i, j < i: position i (i - 1) / 2 + j
    Z = np.einsum("bik,bjk->bij", feat, feat)
    Zabs = np.einsum("bik,bjk->bij", np.abs(feat), np.abs(feat))
    got = R.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, :D], xn.astype(np.float64))
    assert (got[:, Wd:] == 0).all()
    err_f = np.abs(got[:, D:Wd] - Z[:, li, lj])
    bound_f = (D + 1) * u * Zabs[:, li, lj]
    print("forward: worst error / bound %.3g" % float((err_f / bound_f).max()))
    assert (err_f <= bound_f).all()
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
    print("backward: worst error / bound %.3g" % float((err_b / bound_b).max()))
    assert (err_b <= bound_b).all()


# ------------------------------------------------------------------------------------------------ 4. bad input
@pytest.mark.parametrize("D", [16, 64])
def test_out_of_range_ids_are_reported_and_give_the_zero_row(D):
    from dlrm_amd import ops
    B, F = 50, 4
    ws = tables(3, D)
    rows = ROWS[:3]
    rng = np.random.default_rng(5)
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    idx[1][7] = rows[1] + 3            # too large
    idx[2][31] = -1                    # negative
    offs = [torch.arange(B, device=dev()) for _ in rows]

    def bags():
        return ops.BagBatch(offs, [to_dev(i) for i in idx])
    x = x_with_zeros_and_negatives(B, D)
    ldr = ldr_of(F, D, 0)
    dR = dR_of(B, F, D, 0)
    ops.check_index_errors(sync=True)
    # the two-kernel form: its lookup reports the same ids
    E = pooled(ws, bags(), B, D)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd((x, E), D, 0, dR, (dx_ref, dE_ref))
    ops.check_index_errors(sync=True)
    # forward
    R = torch.full((B, ldr), float("nan"), device=dev())
    ops.interact_fwd_gather_narrow(x, ws, bags(), D, 0, R)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(R, ref)
    # pairs (2, 0) and (3, 0) of the bad samples: x . zero row = +0.0
    zero_bits = R[[7, 31], [D + 1, D + 3]].view(torch.int32)
    assert bool((zero_bits == 0).all())
    ops.check_index_errors(sync=True)            # reported once
    # backward: the gradient row of the bad lookup is written like any other
    dx, dE = torch.full((B, D), float("nan"), device=dev()), torch.full((B, 3 * D), float("nan"), device=dev())
    ops.interact_bwd_gather_narrow(x, ws, bags(), D, 0, dR, dx, dE)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert not torch.isnan(dE).any()
    assert same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("D", [16, 64])
def test_broken_bag_start_is_reported(D):
    from dlrm_amd import ops
    B = 40
    ws = tables(2, D)
    rows = ROWS[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    bags = ops.BagBatch([torch.arange(B, device=dev()), to_dev(off)], [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows])
    x = torch.randn((B, D), device=dev())
    R = torch.empty((B, ldr_of(3, D, 0)), device=dev())
    ops.check_index_errors(sync=True)
    ops.interact_fwd_gather_narrow(x, ws, bags, D, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, 2 * D), device=dev())
    ops.interact_bwd_gather_narrow(x, ws, bags, D, 0, dR_of(B, 3, D, 0), dx, dE)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)


def test_refused_operands():
    from dlrm_amd import ops
    B, D = 8, 16
    w = torch.randn((10, D), device=dev())
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, D, 0)), device=dev())
    dR = dR_of(B, 2, D, 0)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, D), device=dev())
    ops.interact_fwd_gather_narrow(x, [w], bags, D, 0, R)                       # (the operands are fine as they stand)
    ops.interact_bwd_gather_narrow(x, [w], bags, D, 0, dR, dx, dE)
    # other widths: the narrow kernels refuse D = 128 and D = 48, the D = 128 kernels keep refusing D = 16
    for d in (128, 48):
        wd, xd = torch.zeros((10, d), device=dev()), torch.zeros((B, d), device=dev())
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_fwd_gather_narrow(xd, [wd], bags, d, 0, torch.empty((B, d + 4), device=dev()))
        with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
            ops.interact_bwd_gather_narrow(xd, [wd], bags, d, 0, torch.zeros((B, d + 4), device=dev()), torch.empty((B, d), device=dev()),
                                           torch.empty((B, d), device=dev()))
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather(x, [w], bags, D, 0, R)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather(x, [w], bags, D, 0, dR, dx, dE)
    # an unaligned table: a view at a 4-byte offset
    raw = torch.empty(10 * D + 1, device=dev())
    odd = raw[1:].view(10, D)
    odd.copy_(w)
    assert odd.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather_narrow(x, [odd], bags, D, 0, R)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather_narrow(x, [odd], bags, D, 0, dR, dx, dE)
    # per-sample weights
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_fwd_gather_narrow(x, [w], wbags, D, 0, R)
    with pytest.raises(RuntimeError, match="per-sample weights"):
        ops.interact_bwd_gather_narrow(x, [w], wbags, D, 0, dR, dx, dE)
    # nnz != B
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_fwd_gather_narrow(x, [w], mbags, D, 0, R)
    with pytest.raises(RuntimeError, match="exactly one lookup per bag"):
        ops.interact_bwd_gather_narrow(x, [w], mbags, D, 0, dR, dx, dE)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 5. predicates
@pytest.mark.parametrize("D", [16, 64])
def test_launch_predicates(D):
    """the fused kernels and the three launches of the two-kernel form, each behind (flag, nonzero): a launch that must not run leaves its
    -7.0-filled output untouched, the other gives the unpredicated bits"""
    from dlrm_amd import ops
    B, F = 70, 5
    T = F - 1
    ws = tables(T, D)
    bags, _ = onehot_bags(np.random.default_rng(8), ROWS[:T], B)
    x = x_with_zeros_and_negatives(B, D)
    ldr = ldr_of(F, D, 0)
    dR = dR_of(B, F, D, 0)
    E_ref = pooled(ws, bags, B, D)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_ref), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E_ref), D, 0, dR, (dx_ref, dE_ref))
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())

    def filled(*shape):
        return torch.full(shape, -7.0, device=dev())
    for flag, nonzero, runs in ((zero, 0, True), (one, 1, True), (zero, 1, False), (one, 0, False)):
        p = (flag, nonzero)
        R, dx, dE = filled(B, ldr), filled(B, D), filled(B, T * D)                      # the fused kernels
        ops.interact_fwd_gather_narrow(x, ws, bags, D, 0, R, pred=p)
        ops.interact_bwd_gather_narrow(x, ws, bags, D, 0, dR, dx, dE, pred=p)
        E, R2, dx2, dE2 = filled(B, T * D), filled(B, ldr), filled(B, D), filled(B, T * D)   # the two-kernel form
        ops.emb_fwd(ws, bags, E, pred=p)
        ops.interact_fwd((x, E_ref), D, 0, R2, pred=p)
        ops.interact_bwd((x, E_ref), D, 0, dR, (dx2, dE2), pred=p)
        ops.check_index_errors(sync=True)
        if runs:
            assert same_bits(R, ref) and same_bits(dx, dx_ref) and same_bits(dE, dE_ref)
            assert same_bits(E, E_ref) and same_bits(R2, ref) and same_bits(dx2, dx_ref) and same_bits(dE2, dE_ref)
        else:
            assert all(bool((t == -7.0).all()) for t in (R, dx, dE, E, R2, dx2, dE2))


# ------------------------------------------------------------------------------------------------ 6. the model
CRITEO_LIKE = [1460, 583, 2000, 1999, 305, 24, 1200, 633, 3, 931, 1500, 2000, 1890, 27, 1040, 1800, 10, 563, 201, 4, 2000, 18, 15, 1300, 105, 1420]
CONFIGS = {"d16_t26": (16, CRITEO_LIKE), "d64_t3": (64, CRITEO_LIKE[:3])}


def model(cfg, on):
    import dlrm_amd
    from dlrm_amd import ops
    d, ln_emb = CONFIGS[cfg]
    np.random.seed(3)
    torch.manual_seed(3)
    F = len(ln_emb) + 1
    m = dlrm_amd.DLRM_Net(d, np.asarray(ln_emb), np.asarray([13, 32, d]), np.asarray([d + F * (F - 1) // 2, 32, 1]), "dot",
                          sigmoid_top=1, loss_function="bce").to(dev())
    m.fuse_narrow_interact = on
    m.emb_update_mode = ops.UPD_SORTED
    return m


def batch(cfg, seed, B, state="tagged"):
    from dlrm_amd import ops
    ln_emb = CONFIGS[cfg][1]
    rng = np.random.default_rng(seed)
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) for _ in ln_emb]
    lS_i = [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in ln_emb]
    target = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    if state == "tagged":
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    if state == "ragged":
        lS_o[1][17] = 16                # bag 16 has two lookups, bag 17 none: nnz == B, not one lookup per bag
    return X, lS_o, lS_i, target


class Counted:
    """wraps the ops of both forms: which path did the model take"""
    NAMES = ("interact_fwd_gather_narrow", "interact_bwd_gather_narrow", "emb_fwd", "interact_fwd", "interact_bwd")

    def __init__(self, monkeypatch):
        from dlrm_amd import ops
        self.n = {k: 0 for k in self.NAMES}
        self.preds = {k: [] for k in self.NAMES}
        self.capturing = {k: 0 for k in self.NAMES}
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, f0):
        def f(*a, **k):
            self.n[name] += 1
            self.preds[name].append(k.get("pred"))
            if torch.cuda.is_current_stream_capturing():
                self.capturing[name] += 1
            return f0(*a, **k)
        return f

    def counts(self):
        return tuple(self.n[k] for k in self.NAMES)


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
        assert same_bits(ea.weight, eb.weight), "table %d" % t
        if oa is not None:
            sa, sb = oa.state[ea.weight]["momentum"], ob.state[eb.weight]["momentum"]
            assert same_bits(sa, sb), "accumulator %d" % t
    for tower in ("bot_l", "top_l"):
        for pa, pb in zip(getattr(a, tower).parameters(), getattr(b, tower).parameters()):
            assert same_bits(pa, pb), tower


@pytest.mark.parametrize("state", ["tagged", "fresh", "ragged"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("cfg", ["d16_t26", "d64_t3"])
def test_model_gives_the_bits_of_the_two_kernel_form(cfg, B, optimizer, state, monkeypatch):
    """tagged: producer-tagged offsets -> the fused kernels alone.  fresh: offsets nobody vouched for -> the fused kernels behind (flag, 0), the
    two-kernel form behind (flag, 1), forward and backward.  ragged: nnz == B with an empty bag next to a two-lookup bag -> the results of
    the attribute-off model (the lookup reports nothing: a ragged batch is legal input of the two-kernel form)."""
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedRWSAdagrad, FusedSGD
    on, off = model(cfg, True), model(cfg, False)
    before = [e.weight.detach().clone() for e in on.emb_l]

    def opt_of(m):
        return FusedSGD(m.parameters(), lr=0.5) if optimizer == "sgd" else FusedRWSAdagrad(m.parameters(), lr=0.05)
    o_on, o_off = opt_of(on), opt_of(off)
    X, lS_o, lS_i, target = batch(cfg, 11 + B, B, state)
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, o_off, X, lS_o, lS_i, target)
    ops.check_index_errors(sync=True)
    if state != "tagged":
        lS_o = [o.clone() for o in lS_o]              # fresh tensor objects: no verdict is cached for them
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert same_bits(got, want)
    if state == "tagged":
        assert calls.counts() == (1, 0, 0, 0, 0) and calls.preds["interact_fwd_gather_narrow"] == [None]
    else:
        assert calls.counts() == (1, 0, 1, 1, 0)
        assert calls.preds["interact_fwd_gather_narrow"][0][1] == 0 and calls.preds["emb_fwd"][0][1] == 1 and calls.preds["interact_fwd"][0][1] == 1
    if state != "tagged":
        lS_o = [o.clone() for o in lS_o]
    calls = Counted(monkeypatch)
    l_on = one_step(on, o_on, X, lS_o, lS_i, target)
    ops.check_index_errors(sync=True)
    if state == "tagged":
        assert calls.counts() == (1, 1, 0, 0, 0)
    else:
        assert calls.counts() == (1, 1, 1, 1, 1)
        assert calls.preds["interact_bwd_gather_narrow"][0][1] == 0 and calls.preds["interact_bwd"][0][1] == 1
    assert l_on == l_off
    if optimizer == "adagrad":
        same_state(on, off, o_on, o_off)
    else:
        same_state(on, off)
    assert any(not same_bits(w0, e.weight) for w0, e in zip(before, on.emb_l))       # (the step moved the tables)


def test_attribute_off_never_calls_the_narrow_ops(monkeypatch):
    off = model("d16_t26", False)
    X, lS_o, lS_i, _ = batch("d16_t26", 5, 64)
    calls = Counted(monkeypatch)
    predict(off, X, lS_o, lS_i)
    assert calls.counts() == (0, 0, 1, 1, 0)


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_graphed_step_takes_the_two_kernel_form(monkeypatch):
    """GraphedTrainStep proves offsets for the D = 128 shapes only: while a graph is being captured the narrow branch is not entered, and the
    graphed step of the attribute-on model is the graphed step of the attribute-off model, bit for bit (deterministic embedding update)"""
    from dlrm_amd import ops
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedSGD
    cfg, B = "d16_t26", 64
    results = []
    for attr in (False, True):
        m = model(cfg, attr)
        m.emb_update_mode = ops.UPD_DETERMINISTIC
        opt = FusedSGD(m.parameters(), lr=0.5)
        calls = Counted(monkeypatch) if attr else None
        step = GraphedTrainStep(m, opt, warmup=2)
        losses = []
        for s in range(5):
            X, lS_o, lS_i, target = batch(cfg, 70 + s, B, "fresh")
            losses.append(float(step(X, lS_o, lS_i, target)))
        torch.cuda.synchronize()
        ops.check_index_errors(sync=True)
        assert step.captures == 1
        if attr:
            assert calls.capturing["interact_fwd_gather_narrow"] == 0 and calls.capturing["interact_bwd_gather_narrow"] == 0
            assert calls.capturing["emb_fwd"] >= 1 and calls.capturing["interact_fwd"] >= 1 and calls.capturing["interact_bwd"] >= 1
        results.append((losses, m))
        monkeypatch.undo()
    assert results[0][0] == results[1][0]
    same_state(results[0][1], results[1][1])
