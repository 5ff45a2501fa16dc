"""Fused lookup + interaction over quotient-remainder tables, forward and backward: dlrm_interact_fwd_gather_qr / dlrm_interact_bwd_gather_qr /
dlrm_emb_fwd_qr_pred / dlrm_emb_qr_bwd_split_pred through dlrm_amd.ops, and DLRM_Net.fuse_qr_interact.

  * op level: R, dx and the gradient buffer of the virtual table list are BIT-IDENTICAL to the two-kernel form (ops.emb_fwd_qr into a feature
    buffer, ops.interact_fwd / ops.interact_bwd over it, ops.emb_qr_bwd_split with the sums that forward saved) and, for in-range ids, to the
    fp32 fused kernels on tables materialised row by row with the element formula; one test is independent of the project's kernels
    (float64 numpy);
  * model level: fuse_qr_interact = True gives the prediction bits, the loss and — after one SGD step — the weight_q / weight_r / plain
    table bits and the tower parameters of fuse_qr_interact = False.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_qr_emb_host as H
from conftest import load_golden, params_with_prefix
from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = 128
ROWS = [1, 37, 2000, 3, 513, 1200, 2, 64, 1999, 17, 300, 5, 1024, 77, 2000, 9, 450, 31, 1500, 4, 800, 129, 11, 1777, 256, 60]      # 26 tables
COLL = [4, 0, 3, 1, 7, 0, 4, 3, 0, 7, 1, 4, 0, 3, 7, 4, 0, 1, 3, 0, 7, 4, 3, 0, 1, 7]                                              # 0: a plain table
# -0.0, fp32 subnormals of both signs, +0.0, the smallest normal, the largest subnormal
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


def host_tables():
    """(weight_q or plain weight, weight_r or None) per table, uniform in [-1, 1].  Row 0 of table 0's weight_q (QR, c = 4) and of table 1
    (plain) carry -0.0 and subnormals in their first columns; the whole weight_r of table 2 (c = 3) consists of them."""
    if "host" not in _tables:
        rng = np.random.default_rng(2025)
        hs = []
        for t, (n, c) in enumerate(zip(ROWS, COLL)):
            w = rng.uniform(-1.0, 1.0, size=(H.rows_q(n, c) if c else n, D)).astype(np.float32)
            wr = rng.uniform(-1.0, 1.0, size=(c, D)).astype(np.float32) if c else None
            if t in (0, 1):
                w[0, :SPECIAL.size] = SPECIAL
            if t == 2:
                wr[:] = np.tile(SPECIAL, D // SPECIAL.size)[None, :]
            hs.append((w, wr))
        _tables["host"] = hs
    return _tables["host"]


def tables(T):
    """device tensors (weights, weights_r) of the first T tables"""
    if "dev" not in _tables:
        hs = host_tables()
        _tables["dev"] = ([to_dev(w) for w, _ in hs], [None if r is None else to_dev(r) for _, r in hs])
    W, Wr = _tables["dev"]
    return W[:T], Wr[:T]


def materialised(T, op):
    """the [n, D] fp32 table of every category, row by row with the element formula: fmaf(1, Wq[q], +0) op fmaf(1, Wr[r], +0), each rounded
    once (numpy float32 arithmetic is IEEE, subnormals included); fmaf(1, W[id], +0) for a plain table"""
    key = "mat_" + op
    if key not in _tables:
        out = []
        zero = np.float32(0.0)
        for (w, wr), n, c in zip(host_tables(), ROWS, COLL):
            if not c:
                out.append(to_dev(w + zero))
                continue
            q, r, ok = H.qr_split(np.arange(n), n, c)
            assert ok.all() and np.array_equal(q, np.arange(n) // c)
            sq, sr = w[q] + zero, wr[r] + zero
            out.append(to_dev(sq * sr if op == "mult" else sq + sr))
        _tables[key] = out
    return _tables[key][:T]


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


def n_virtual(coll):
    return len(coll) + sum(1 for c in coll if c)


def pooled(W, Wr, rows, coll, op, bags, B, keep=True):
    """the [B, T*D] fp32 buffer of the two-kernel form and the sums its forward keeps for the backward"""
    from dlrm_amd import ops
    E = torch.empty((B, len(W) * D), device=dev())
    saved = torch.empty((B, 2 * D * sum(1 for c in coll if c)), device=dev()) if (keep and op == "mult" and any(coll)) else None
    ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, E, saved)
    return E, saved


def two_kernel_backward(x, E, saved, coll, op, m, dR):
    from dlrm_amd import ops
    B, T = x.size(0), len(coll)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E), D, m, dR, (dx, dE))
    return dx, ops.emb_qr_bwd_split(coll, op, D, dE, saved)


def x_with_zeros_and_negatives(B):
    x = torch.randn((B, D), device=dev())
    x[:, 5::16] = 0.0
    return x


def dR_of(B, F, mode):
    from dlrm_amd import ops
    Wd = ops.interact_out_width(F, D, mode)
    dR = torch.zeros((B, ldr_of(F, mode)), device=dev())
    dR[:, :Wd] = torch.randn((B, Wd), device=dev())
    return dR


# ------------------------------------------------------------------------------------------------ 1. the forward grid
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_forward_bit_identity_grid(F, idx_dtype, op):
    """B = 1 / 3 / 5 leave waves and workgroups without a sample; B = 5000 exceeds twice the samples one pass of the grid covers (256
    workgroups x 4 at F > 16, 512 x 4 at F <= 16): some waves run the prologue, a steady-state iteration and the clamped tail, others one
    iteration fewer.  F = 16 / 17 straddle the NB = 1 / 2 instantiations."""
    from dlrm_amd import ops
    T = F - 1
    W, Wr = tables(T)
    rows, coll = ROWS[:T], COLL[:T]
    mat = materialised(T, op)
    rng = np.random.default_rng(F * 10)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000, 5000):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = torch.randn((B, D), device=dev())
        E, _ = pooled(W, Wr, rows, coll, op, bags, B, keep=False)
        for mode in (0, 1, 2):
            ldr = ldr_of(F, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref = torch.empty((B, ldr), device=dev())
            ops.interact_fwd((x, E), D, mode, ref)
            ref32 = torch.empty((B, ldr), device=dev())
            ops.interact_fwd_gather(x, mat, bags, D, mode, ref32)
            buf1, R1 = guarded(B, ldr)
            buf2, R2 = guarded(B, ldr)
            ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, mode, R1)
            ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert same_bits(R1, ref), what + ": the two-kernel form"
            assert same_bits(R1, ref32), what + ": the fp32 fused kernel on the materialised tables"
            assert same_bits(R1, R2), what + ": two runs differ"
            assert canaries_intact(buf1, buf2), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. the backward grid
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_backward_bit_identity_grid(F, idx_dtype, op):
    from dlrm_amd import ops
    T = F - 1
    W, Wr = tables(T)
    rows, coll = ROWS[:T], COLL[:T]
    Tv = n_virtual(coll)
    rng = np.random.default_rng(F * 10 + 1)
    ops.check_index_errors(sync=True)
    for B in (1, 3, 5, 64, 1000, 5000):
        bags, _ = onehot_bags(rng, rows, B, idx_dtype)
        x = x_with_zeros_and_negatives(B)
        E, saved = pooled(W, Wr, rows, coll, op, bags, B)
        for mode in (0, 1, 2):
            dR = dR_of(B, F, mode)
            for relu in ((0, ops.INTERACT_RELU_X) if mode == 0 else (0,)):
                m = mode | relu
                dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, m, dR)
                outs = []
                for _ in range(2):
                    bx, dx = guarded(B, D)
                    bg, gout = guarded(B, Tv * D)
                    ops.interact_bwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, m, dR, dx, gout)
                    outs.append((bx, dx, bg, gout))
                ops.check_index_errors(sync=True)
                (bx, dx, bg, gout), (bx2, dx2, bg2, gout2) = outs
                what = "B=%d mode=%d relu=%d" % (B, mode, relu)
                assert not torch.isnan(dx).any() and not torch.isnan(gout).any(), what
                assert same_bits(dx, dx_ref) and same_bits(gout, g_ref), what + ": the two-kernel form"
                assert same_bits(dx, dx2) and same_bits(gout, gout2), what + ": two runs differ"
                assert canaries_intact(bx, bg, bx2, bg2), what
                if relu:
                    assert bool((dx[x <= 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------ 3. independent of the project's kernels
@pytest.mark.parametrize("op", ["mult", "add"])
def test_against_float64_numpy(op):
    """R, dx, gout against oracle.interact_fwd / oracle.interact_bwd (float64) on rows gathered and composed in numpy, at the bound of
    tests/test_gpu_bf16_interact.py::test_against_float64_numpy (forward rtol 1e-5, atol 1e-5; backward rtol 1e-5, atol 2e-5), with that
    test's 0.25 scale of the table values for its reason.  The composed rows are no larger than that test's rows (products of two
    N(0, 0.25^2) values, or sums of two N(0, 0.125^2) values), and gout = dE * (a row of scale 0.25) is no larger than dE."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows, coll = ROWS[:T], COLL[:T]
    Tv = n_virtual(coll)
    rng = np.random.default_rng(303)
    scale = 0.25 if op == "mult" else 0.125
    hs = []
    for n, c in zip(rows, coll):
        if c:
            hs.append(((scale * rng.standard_normal((H.rows_q(n, c), D))).astype(np.float32), (scale * rng.standard_normal((c, D))).astype(np.float32)))
        else:
            hs.append(((0.25 * rng.standard_normal((n, D))).astype(np.float32), None))
    W, Wr = [to_dev(w) for w, _ in hs], [None if r is None else to_dev(r) for _, r in hs]
    bags, idx = onehot_bags(np.random.default_rng(33), rows, B)
    x = to_dev(rng.standard_normal((B, D)).astype(np.float32))
    Wd = ops.interact_out_width(F, D, 0)
    ldr = ldr_of(F, 0)
    dRn = rng.standard_normal((B, Wd)).astype(np.float32)
    dR = torch.zeros((B, ldr), device=dev())
    dR[:, :Wd] = to_dev(dRn)
    R = torch.empty((B, ldr), device=dev())
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, Tv * D), device=dev())
    ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, 0, R)
    ops.interact_bwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout)
    ops.check_index_errors(sync=True)
    feat = np.empty((B, F, D), dtype=np.float64)
    feat[:, 0] = x.cpu().numpy()
    comps = []
    for t, ((w, wr), c) in enumerate(zip(hs, coll)):
        if c:
            sq, sr = w[idx[t] // c].astype(np.float64), wr[idx[t] % c].astype(np.float64)
            feat[:, 1 + t] = sq * sr if op == "mult" else sq + sr
            comps.append((sq, sr))
        else:
            feat[:, 1 + t] = w[idx[t]]
            comps.append(None)
    want = O.interact_fwd(feat, False)
    dwant = O.interact_bwd(feat, dRn, False)
    gwant = []
    for t, cs in enumerate(comps):
        g = dwant[:, 1 + t]
        if cs is None:
            gwant.append(g)
        else:
            gwant += [g * cs[1], g * cs[0]] if op == "mult" else [g, g]
    gwant = np.concatenate(gwant, axis=1)
    got = R.cpu().numpy()

    def ratio(g, w, atol):
        return float((np.abs(g - w) / (atol + 1e-5 * np.abs(w))).max())
    gx, gg = dx.cpu().numpy(), gout.cpu().numpy()
    print("worst error / (atol + rtol |want|): forward %.3g, dx %.3g, gout %.3g"
          % (ratio(got[:, :Wd], want, 1e-5), ratio(gx, dwant[:, 0], 2e-5), ratio(gg, gwant, 2e-5)))
    np.testing.assert_allclose(got[:, :Wd], want, rtol=1e-5, atol=1e-5)
    assert (got[:, Wd:] == 0).all()
    np.testing.assert_allclose(gx, dwant[:, 0], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(gg, gwant, rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 4. the float32 quotient above 2^24
BIG_N, BIG_C = 18_750_000, 4          # weight_q: 4,687,500 rows of 512 bytes = 2.4 GB, never filled as a whole


@pytest.mark.parametrize("op", ["mult", "add"])
def test_large_table_rows_follow_the_float32_quotient(op):
    """ids above 2^24 whose float32 quotient is not id // 4, and id n - 1 = 18,749,999, which float32 rounds to 18,750,000: its quotient
    4,687,500 = ceil(n / c) is no row — refused and reported.  Only the weight_q rows the lookups name are written, from a small table."""
    from dlrm_amd import ops
    B = 1000
    nq = H.rows_q(BIG_N, BIG_C)
    rng = np.random.default_rng(44)
    ids = rng.integers(2 ** 24, BIG_N, size=B).astype(np.int64)
    ids[0], ids[1], ids[-1] = BIG_N - 2, 0, BIG_N - 1
    q, r, ok = H.qr_split(ids, BIG_N, BIG_C)
    assert np.array_equal(q, (torch.from_numpy(ids) / BIG_C).long().numpy())
    assert int((q[ok] != ids[ok] // BIG_C).sum()) > B // 16                 # the test can tell the two mappings apart
    assert int((~ok).sum()) == 1 and not ok[-1] and q[-1] == nq
    assert int(q[ok].max()) * 512 > 2 ** 31
    uniq = np.unique(q[ok])
    small = torch.rand((uniq.size, D), device=dev()) - 0.5
    big = torch.empty((nq, D), device=dev())
    big.index_copy_(0, to_dev(uniq), small)
    wr = torch.rand((BIG_C, D), device=dev()) - 0.5
    rows, coll = [BIG_N], [BIG_C]
    want_msg = r"index %d, rows %d" % (BIG_N - 1, BIG_N)
    try:
        ops.check_index_errors(sync=True)
        for idx_dtype in (torch.int64, torch.int32):
            bags = ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype)], [to_dev(ids, idx_dtype)])
            x = x_with_zeros_and_negatives(B)
            ldr = ldr_of(2, 0)
            E, saved = pooled([big], [wr], rows, coll, op, bags, B)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            # the rows really are the float-quotient rows of the small table; the refused lookup gives the zero row
            okd, zeros = to_dev(ok)[:, None], torch.zeros((B, D), device=dev())
            sq = torch.where(okd, small[to_dev(np.searchsorted(uniq, np.where(ok, q, uniq[0])))] + 0.0, zeros)
            sr = torch.where(okd, wr[to_dev(np.where(ok, r, 0))] + 0.0, zeros)
            assert same_bits(E, sq * sr if op == "mult" else sq + sr)
            ref, R = torch.empty((B, ldr), device=dev()), torch.full((B, ldr), float("nan"), device=dev())
            ops.interact_fwd((x, E), D, 0, ref)
            dR = dR_of(B, 2, 0)
            dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, 0, dR)
            ops.interact_fwd_gather_qr(x, [big], [wr], rows, coll, op, bags, D, 0, R)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            dx, gout = torch.full((B, D), float("nan"), device=dev()), torch.full((B, 2 * D), float("nan"), device=dev())
            ops.interact_bwd_gather_qr(x, [big], [wr], rows, coll, op, bags, D, 0, dR, dx, gout)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            assert same_bits(R, ref)
            assert same_bits(dx, dx_ref) and same_bits(gout, g_ref)
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5. bad input
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_out_of_range_ids_are_reported_and_give_the_zero_row(idx_dtype, op):
    from dlrm_amd import ops
    B, F = 50, 4
    W, Wr = tables(3)
    rows, coll = ROWS[:3], COLL[:3]             # QR (c = 4, n = 1), plain, QR (c = 3)
    Tv = n_virtual(coll)
    rng = np.random.default_rng(5)
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    idx[0][9] = rows[0]                # == n of a QR table: its quotient 0 IS a row of weight_q, the id is still no category
    idx[1][7] = rows[1] + 3            # too large, plain table
    idx[2][31] = -1                    # negative, QR table
    idx[2][40] = rows[2]               # == n
    offs = [torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows]

    def bags():
        return ops.BagBatch(offs, [to_dev(i, idx_dtype) for i in idx])
    x = x_with_zeros_and_negatives(B)
    ldr = ldr_of(F, 0)
    dR = dR_of(B, F, 0)
    ops.check_index_errors(sync=True)
    # the two-kernel form: its lookup reports the same ids
    E, saved = pooled(W, Wr, rows, coll, op, bags(), B)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert bool((E[9, :D].view(torch.int32) == 0).all()) and bool((E[31, 2 * D:].view(torch.int32) == 0).all())
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E), D, 0, ref)
    dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, 0, dR)
    ops.check_index_errors(sync=True)
    # forward
    R = torch.full((B, ldr), float("nan"), device=dev())
    ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, op, bags(), D, 0, R)
    with pytest.raises(IndexError, match=r"index (1|40|-1|2000), rows (1|37|2000) "):
        ops.check_index_errors(sync=True)
    assert same_bits(R, ref)
    # pairs (1, 0), (2, 0), (3, 0) of the bad samples: x . zero row = +0.0
    zero_bits = R[[9, 7, 31, 40], [D + 0, D + 1, D + 3, D + 3]].view(torch.int32)
    assert bool((zero_bits == 0).all())
    ops.check_index_errors(sync=True)            # reported once
    # backward: gout as the two-kernel form writes it (dout * (+0) for "mult", dout for "add", a copy for the plain table)
    dx, gout = torch.full((B, D), float("nan"), device=dev()), torch.full((B, Tv * D), float("nan"), device=dev())
    ops.interact_bwd_gather_qr(x, W, Wr, rows, coll, op, bags(), D, 0, dR, dx, gout)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    assert same_bits(dx, dx_ref) and same_bits(gout, g_ref)
    ops.check_index_errors(sync=True)


def test_broken_bag_start_is_reported():
    from dlrm_amd import ops
    B = 40
    W, Wr = tables(2)
    rows, coll = ROWS[:2], COLL[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    bags = ops.BagBatch([to_dev(off), torch.arange(B, device=dev())], [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows])
    x = torch.randn((B, D), device=dev())
    R = torch.empty((B, ldr_of(3, 0)), device=dev())
    ops.check_index_errors(sync=True)
    ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, "mult", bags, D, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd_gather_qr(x, W, Wr, rows, coll, "mult", bags, D, 0, dR_of(B, 3, 0), dx, gout)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 6. predicates
@pytest.mark.parametrize("op", ["mult", "add"])
def test_launch_predicates(op):
    from dlrm_amd import ops
    B, F = 70, 6
    T = F - 1
    W, Wr = tables(T)
    rows, coll = ROWS[:T], COLL[:T]
    Tv, nq = n_virtual(coll), sum(1 for c in coll if c)
    bags, _ = onehot_bags(np.random.default_rng(8), rows, B)
    x = x_with_zeros_and_negatives(B)
    ldr = ldr_of(F, 0)
    dR = dR_of(B, F, 0)
    E_ref, sv_ref = pooled(W, Wr, rows, coll, op, bags, B)
    if sv_ref is None:
        sv_ref = torch.empty((B, 2 * nq * D), device=dev())
        ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, torch.empty_like(E_ref), sv_ref)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_ref), D, 0, ref)
    dE_ref = torch.empty((B, T * D), device=dev())
    dx_ref = torch.empty((B, D), device=dev())
    ops.interact_bwd((x, E_ref), D, 0, dR, (dx_ref, dE_ref))
    g_ref = ops.emb_qr_bwd_split(coll, op, D, dE_ref, sv_ref)
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())
    for flag, nonzero, runs in ((zero, 0, True), (one, 1, True), (zero, 1, False), (one, 0, False)):
        nan = float("nan")
        R = torch.full((B, ldr), nan, device=dev())
        E, sv = torch.full((B, T * D), nan, device=dev()), torch.full((B, 2 * nq * D), nan, device=dev())
        dx, gout, gsplit = torch.full((B, D), nan, device=dev()), torch.full((B, Tv * D), nan, device=dev()), torch.full((B, Tv * D), nan, device=dev())
        ops.interact_fwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, 0, R, pred=(flag, nonzero))
        ops.interact_bwd_gather_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout, pred=(flag, nonzero))
        ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, E, sv, pred=(flag, nonzero))
        ops.emb_qr_bwd_split(coll, op, D, dE_ref, sv_ref, gsplit, pred=(flag, nonzero))
        ops.check_index_errors(sync=True)
        if runs:
            assert same_bits(R, ref) and same_bits(E, E_ref) and same_bits(sv, sv_ref)
            assert same_bits(dx, dx_ref) and same_bits(gout, g_ref) and same_bits(gsplit, g_ref)
        else:
            assert all(bool(torch.isnan(t).all()) for t in (R, E, sv, dx, gout, gsplit))


# ------------------------------------------------------------------------------------------------ 7. refusals
E_ARG, E_RANGE, E_MODE = -1, -3, -4           # include/dlrm_hip.h


def raw_call(which, x, W, Wr, rows, coll, op_code, bags, mode, R_or_dR, dx=None, gout=None, B=None, d=D):
    """the C entry point itself, with operands ops.* would refuse first (an unknown op, a null weight_r)"""
    from dlrm_amd import _lib, ops
    lib = _lib.load()
    T = len(W)
    wp = _lib.ptr_array([w.data_ptr() for w in W])
    wrp = _lib.ptr_array([0 if r is None else r.data_ptr() for r in Wr])
    common = (x.size(0) if B is None else B, 1 + T, d, C.c_void_p(x.data_ptr()), ops._ld(x), wp, wrp, _lib.i64_array(rows),
              (C.c_int * T)(*coll), op_code, bags._idx, bags._off, bags.idx_bits, mode, C.c_void_p(R_or_dR.data_ptr()), ops._ld(R_or_dR))
    st = ops._stream(x)
    if which == "fwd":
        return lib.dlrm_interact_fwd_gather_qr(*common, None, None, 0, st)
    return lib.dlrm_interact_bwd_gather_qr(*common, C.c_void_p(dx.data_ptr()), ops._ld(dx), C.c_void_p(gout.data_ptr()), ops._ld(gout), None,
                                           None, 0, st)


def test_refused_operands():
    from dlrm_amd import ops
    B = 8
    assert ops.gather_qr_ok(27, 128) and ops.gather_qr_ok(2, 128)
    assert not ops.gather_qr_ok(27, 64) and not ops.gather_qr_ok(28, 128)
    g = torch.Generator(device=dev()).manual_seed(1)
    wq, wr = torch.rand((25, D), device=dev(), generator=g), torch.rand((4, D), device=dev(), generator=g)
    rows, coll = [100], [4]
    bags = ops.BagBatch([torch.arange(B, device=dev())], [torch.arange(B, device=dev()) * 3])
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, ldr_of(2, 0)), device=dev())
    dR = dR_of(B, 2, 0)
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, 2 * D), device=dev())
    ops.interact_fwd_gather_qr(x, [wq], [wr], rows, coll, "mult", bags, D, 0, R)                       # (the operands are fine as they stand)
    ops.interact_bwd_gather_qr(x, [wq], [wr], rows, coll, "mult", bags, D, 0, dR, dx, gout)
    assert raw_call("fwd", x, [wq], [wr], rows, coll, 0, bags, 0, R) == 0
    assert raw_call("bwd", x, [wq], [wr], rows, coll, 1, bags, 0, dR, dx, gout) == 0

    def both(match, x_=x, W=(wq,), Wr_=(wr,), R_=R, dR_=dR, dx_=dx, gout_=gout, bags_=bags, rows_=rows, coll_=coll, d=D):
        with pytest.raises(RuntimeError, match=match):
            ops.interact_fwd_gather_qr(x_, list(W), list(Wr_), rows_, coll_, "mult", bags_, d, 0, R_)
        with pytest.raises(RuntimeError, match=match):
            ops.interact_bwd_gather_qr(x_, list(W), list(Wr_), rows_, coll_, "add", bags_, d, 0, dR_, dx_, gout_)
    # D = 64
    both("DLRM_E_MODE", x_=x[:, :64].contiguous(), W=(wq[:, :64].contiguous(),), Wr_=(wr[:, :64].contiguous(),), R_=torch.empty((B, 68), device=dev()),
         dR_=torch.zeros((B, 68), device=dev()), dx_=torch.empty((B, 64), device=dev()), gout_=torch.empty((B, 128), device=dev()), d=64)
    # F = 28
    bags27 = ops.BagBatch([torch.arange(B, device=dev())] * 27, [torch.zeros(B, dtype=torch.int64, device=dev())] * 27)
    both("DLRM_E_MODE", W=(wq,) * 27, Wr_=(wr,) * 27, rows_=rows * 27, coll_=coll * 27, bags_=bags27, R_=torch.empty((B, ldr_of(28, 0)), device=dev()),
         dR_=torch.zeros((B, ldr_of(28, 0)), device=dev()), gout_=torch.empty((B, 54 * D), device=dev()))

    def shifted(t, by=1):
        """a copy of t at a 4-byte offset"""
        raw = torch.empty(t.numel() + by, device=dev())
        v = raw[by:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * by
        return v
    # misaligned weight_q / weight_r / plain table / x / R, dR, dx, gout
    assert ops.qr_tables_aligned([wq], [wr]) and not ops.qr_tables_aligned([shifted(wq)], [wr]) and not ops.qr_tables_aligned([wq], [shifted(wr)])
    both("DLRM_E_MODE", W=(shifted(wq),))
    both("DLRM_E_MODE", Wr_=(shifted(wr),))
    both("DLRM_E_MODE", W=(shifted(torch.rand((100, D), device=dev())),), Wr_=(None,), coll_=[0], gout_=torch.empty((B, D), device=dev()))
    both("DLRM_E_MODE", x_=shifted(x))
    both("DLRM_E_MODE", R_=shifted(R), dR_=shifted(dR))
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather_qr(x, [wq], [wr], rows, coll, "mult", bags, D, 0, dR, shifted(dx), gout)
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_bwd_gather_qr(x, [wq], [wr], rows, coll, "mult", bags, D, 0, dR, dx, shifted(gout))
    # ldr % 4 != 0 (16-byte aligned base, rows 4 * 133 bytes apart)
    odd_ld = torch.zeros((B, ldr_of(2, 0) + 1), device=dev())
    assert odd_ld.data_ptr() % 16 == 0 and odd_ld.stride(0) % 4 == 1
    both("DLRM_E_MODE", R_=odd_ld, dR_=odd_ld)
    # an unknown op, a null weight_r for a QR table, collisions < 0, rows <= 0: DLRM_E_ARG (ops refuses them itself: the C call)
    with pytest.raises(RuntimeError, match="'mult' or 'add'"):
        ops.interact_fwd_gather_qr(x, [wq], [wr], rows, coll, "concat", bags, D, 0, R)
    assert raw_call("fwd", x, [wq], [wr], rows, coll, 2, bags, 0, R) == E_ARG
    assert raw_call("bwd", x, [wq], [wr], rows, coll, -1, bags, 0, dR, dx, gout) == E_ARG
    assert raw_call("fwd", x, [wq], [None], rows, coll, 0, bags, 0, R) == E_ARG
    assert raw_call("bwd", x, [wq], [None], rows, coll, 0, bags, 0, dR, dx, gout) == E_ARG
    assert raw_call("fwd", x, [wq], [wr], rows, [-1], 0, bags, 0, R) == E_ARG
    assert raw_call("fwd", x, [wq], [wr], [0], coll, 0, bags, 0, R) == E_ARG
    # more than 0xFFFFFFFF rows of weight_q (nothing is launched: the pointers are never followed)
    assert raw_call("fwd", x, [wq], [wr], [4 * 0xFFFFFFFF + 1], coll, 0, bags, 0, R) == E_RANGE
    assert raw_call("fwd", x, [wq], [wr], [4 * 0xFFFFFFFF], coll, 0, bags, 0, R) == 0
    assert raw_call("bwd", x, [wq], [None], [0x100000000], [0], 0, bags, 0, dR, dx, gout) == E_RANGE
    # a gout narrower than the virtual table list
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.interact_bwd_gather_qr(x, [wq], [wr], rows, coll, "mult", bags, D, 0, dR, dx, gout[:, :D])
    # per-sample weights, nnz != B
    wbags = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())], [torch.ones(B, device=dev())])
    both("per-sample weights", bags_=wbags)
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2], [torch.zeros(2 * B, dtype=torch.int64, device=dev())])
    both("exactly one lookup per bag", bags_=mbags)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 8. the model
def fixture_case(name="onehot128"):
    d, meta = load_golden("qr_training")
    return d, meta, meta["cases"][name]


def qr_model(fused, mode=None, name="onehot128", **kw):
    """the fixture's model from its stored start parameters"""
    d, meta, case = fixture_case(name)
    m = H.build_qr_model(case, meta["qr_threshold"], params=params_with_prefix(d, name + ".start"), seed=1, **kw).to(dev())
    m.fuse_qr_interact = fused
    if mode is not None:
        m.emb_update_mode = mode
    return m


def fixture_batch(s=0, tagged=True, name="onehot128"):
    from dlrm_amd import ops
    d, meta, case = fixture_case(name)
    X, lS_o, lS_i, T = H.case_batches(d, name, case, meta["steps"])[s]
    lS_o = [to_dev(o) for o in lS_o]
    if tagged:
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    return to_dev(X), lS_o, [to_dev(i) for i in lS_i], to_dev(T)


class Counted:
    """wraps the four ops a QR model may take: which path did it take"""

    NAMES = ("interact_fwd_gather_qr", "interact_bwd_gather_qr", "emb_fwd_qr", "emb_qr_bwd_split")

    def __init__(self, monkeypatch):
        from dlrm_amd import ops
        self.n = dict.fromkeys(self.NAMES, 0)
        self.preds = {k: [] for k in self.NAMES}
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, f0):
        def f(*a, **k):
            self.n[name] += 1
            self.preds[name].append(k.get("pred"))
            return f0(*a, **k)
        return f

    def counts(self):
        return tuple(self.n[k] for k in self.NAMES)


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


def same_parameters(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert any(k.endswith("weight_q") for k in sa) and any(k.endswith("weight_r") for k in sa) and any(k.startswith("emb_l") and k.endswith(".weight") for k in sa)
    for k in sa:
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), k


UPDATE_MODES = ["sorted", "atomic", "deterministic"]


def update_mode(name):
    from dlrm_amd import ops
    return {"sorted": ops.UPD_SORTED, "atomic": ops.UPD_ATOMIC, "deterministic": ops.UPD_DETERMINISTIC}[name]


@pytest.mark.parametrize("mode_name", UPDATE_MODES)
def test_model_takes_the_fused_kernels_and_gives_the_bits_of_the_two_kernel_form(mode_name, monkeypatch):
    """Both models hand the same gradient bits to the same update kernel, so every parameter is compared bit for bit in all three modes."""
    from dlrm_amd import ops
    mode = update_mode(mode_name)
    on, off = qr_model(True, mode), qr_model(False, mode)
    X, lS_o, lS_i, target = fixture_batch(0)
    want = predict(off, X, lS_o, lS_i)
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert calls.counts() == (1, 0, 0, 0) and calls.preds["interact_fwd_gather_qr"] == [None]
    assert same_bits(got, want)
    before = {k: v.clone() for k, v in on.state_dict().items()}
    l_on = one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (2, 1, 0, 0) and calls.preds["interact_bwd_gather_qr"] == [None]
    l_off = one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (2, 1, 1, 1)                  # (the off-model's two-kernel form)
    assert l_on == l_off
    same_parameters(on, off)
    after = on.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in after if k.endswith("weight_q") or k.endswith("weight_r"))   # (the step moved the tables)


@pytest.mark.parametrize("mode_name", UPDATE_MODES)
def test_fused_model_trains_like_the_live_reference(mode_name):
    """the fixture's three steps at the tolerances of tests/test_gpu_qr_emb.py::test_model_trains_like_the_live_reference (its
    train_and_check: losses 1e-5 relative, predictions rtol 2e-5 / atol 1e-6, parameters rtol 1e-4 / atol 2e-6), fuse_qr_interact on.  The
    fixture's offsets are untagged: every step takes the device-flag path."""
    import test_gpu_qr_emb as Q

    def configure(m):
        m.emb_update_mode = update_mode(mode_name)
        m.fuse_qr_interact = True
    model, _, _ = Q.train_and_check("onehot128", configure)
    assert model.fuse_qr_interact


@pytest.mark.parametrize("case", ["untagged", "ragged", "fuse_emb_interact_off"])
def test_other_offsets_states_give_the_bits_of_the_two_kernel_form(case, monkeypatch):
    """untagged: fresh offsets nobody vouched for -> the device-flag path: the fused kernels behind (flag, 0), the two-kernel form behind
    (flag, 1), forward and backward.  ragged: nnz == B with an empty bag next to a two-lookup bag -> the flag path runs the two-kernel
    form.  fuse_emb_interact off: the fused branch is not entered."""
    from dlrm_amd import ops
    on, off = qr_model(True, ops.UPD_DETERMINISTIC), qr_model(False, ops.UPD_DETERMINISTIC)
    X, lS_o, lS_i, target = fixture_batch(1, tagged=False)
    if case == "ragged":
        lS_o[2][17] = 16
    if case == "fuse_emb_interact_off":
        on.fuse_emb_interact = False
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    lS_o = [o.clone() for o in lS_o]                  # fresh tensor objects: no verdict is cached for them
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert same_bits(got, want)
    if case == "fuse_emb_interact_off":
        assert calls.counts() == (0, 0, 1, 0)
    else:
        assert calls.counts() == (1, 0, 1, 0)
        assert calls.preds["interact_fwd_gather_qr"][-1][1] == 0 and calls.preds["emb_fwd_qr"][-1][1] == 1
    lS_o = [o.clone() for o in lS_o]
    l_on = one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target)
    if case == "fuse_emb_interact_off":
        assert calls.counts() == (0, 0, 2, 1)
    else:
        assert calls.counts() == (2, 1, 2, 1)
        assert calls.preds["interact_bwd_gather_qr"][-1][1] == 0 and calls.preds["emb_qr_bwd_split"][-1][1] == 1
    assert l_on == l_off
    same_parameters(on, off)


@pytest.mark.parametrize("case", ["multihot", "cat", "d16", "md"])
def test_other_models_keep_the_two_kernel_form(case, monkeypatch):
    import dlrm_amd
    from dlrm_amd import ops
    rng = np.random.default_rng(41)
    if case == "md":
        import test_md_emb_host as MH
        d, meta = load_golden("md_training")
        mcase = meta["cases"]["onehot128"]              # base dimension 128, one lookup per bag: only the MD tables keep it out

        def build(fused):
            m = MH.build_md_model(mcase, meta["md_threshold"], seed=1).to(dev())
            m.fuse_qr_interact = fused
            return m
        ln_emb, B, hots = mcase["ln_emb"], 48, 1
    elif case == "d16":
        def build(fused):
            return qr_model(fused, name="mult")
        ln_emb, B, hots = fixture_case("mult")[2]["ln_emb"], 48, 1
    elif case == "cat":
        _, meta, c = fixture_case()
        ln_emb, B, hots = c["ln_emb"], 48, 1

        def build(fused):
            np.random.seed(5)
            torch.manual_seed(5)
            m = dlrm_amd.DLRM_Net(c["m_spa"], np.asarray(ln_emb), np.asarray(c["ln_bot"]), np.asarray([c["m_spa"] * (1 + len(ln_emb)), 32, 1]), "cat",
                                  sigmoid_top=1, loss_function="bce", qr_flag=True, qr_operation="mult", qr_collisions=4,
                                  qr_threshold=meta["qr_threshold"]).to(dev())
            m.fuse_qr_interact = fused
            return m
    else:
        def build(fused):
            return qr_model(fused)
        ln_emb, B, hots = fixture_case()[2]["ln_emb"], 48, 3
    on, off = build(True), build(False)
    assert on._has_qr(on.emb_l) == (case != "md")
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) * hots for _ in ln_emb]
    lS_i = [to_dev(rng.integers(0, n, size=B * hots).astype(np.int64)) for n in ln_emb]
    if hots == 1:
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    want = predict(off, X, lS_o, lS_i)
    calls = Counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert calls.counts() == (0, 0, 0 if case == "md" else 1, 0)
    assert same_bits(got, want)


def test_update_in_backward_keeps_the_step_time_update(monkeypatch):
    from dlrm_amd import ops
    on, off = qr_model(True, ops.UPD_DETERMINISTIC), qr_model(False, ops.UPD_DETERMINISTIC)
    on.update_in_backward = True
    presorts = []
    p0 = ops.emb_presort
    monkeypatch.setattr(ops, "emb_presort", lambda *a, **k: presorts.append(1) or p0(*a, **k))
    calls = Counted(monkeypatch)
    o_on, o_off = torch.optim.SGD(on.parameters(), lr=0.1), torch.optim.SGD(off.parameters(), lr=0.1)
    for s in range(2):                                 # (the optimizer is bound at the first step: the second backward could update)
        X, lS_o, lS_i, target = fixture_batch(s)
        assert one_step(on, o_on, X, lS_o, lS_i, target) == one_step(off, o_off, X, lS_o, lS_i, target)
    assert not presorts
    assert calls.counts() == (2, 2, 2, 2)              # two fused steps of `on`, two two-kernel steps of `off`
    same_parameters(on, off)


def test_evaluate_inference_takes_the_fused_forward(monkeypatch):
    from dlrm_amd import evaluate
    on, off = qr_model(True), qr_model(False)
    batches = []
    for s in range(2):
        X, lS_o, lS_i, Tg = fixture_batch(s, tagged=False)
        batches.append((X.cpu(), [o.cpu() for o in lS_o], [i.cpu() for i in lS_i], Tg.cpu()))
    want = evaluate.inference(off, batches, device=dev())
    calls = Counted(monkeypatch)
    got = evaluate.inference(on, batches, device=dev())
    assert calls.n["interact_fwd_gather_qr"] == 2 and calls.n["interact_bwd_gather_qr"] == 0
    assert got == want


@pytest.mark.parametrize("tagged", [True, False])
def test_backward_twice_through_a_retained_graph(tagged):
    """nothing the backward needs is consumed by it (the rows are fetched again; on the device-flag path the sums stay with the node)"""
    from dlrm_amd import ops
    model = qr_model(True)
    X, lS_o, lS_i, T = fixture_batch(0, tagged=tagged)
    E = model.loss_fn(model(X, lS_o, lS_i), T)
    E.backward(retain_graph=True)
    E.backward()
    assert len(model._pending_emb) == 2
    (w1, _, g1, _), (_, _, g2, _) = model._pending_emb
    assert len(w1) == 5 and g1.size(1) == 5 * D            # the virtual table list: q, r, plain, q, r
    assert torch.equal(g1, g2)
    model._pending_emb.clear()
    ops.check_index_errors(sync=True)


def test_a_model_without_qr_tables_gives_the_same_bits_with_the_attribute_set(monkeypatch):
    import dlrm_amd
    from dlrm_amd import ops
    _, _, c = fixture_case()

    def build(fused):
        np.random.seed(7)
        torch.manual_seed(7)
        m = dlrm_amd.DLRM_Net(c["m_spa"], np.asarray(c["ln_emb"]), np.asarray(c["ln_bot"]), np.asarray(c["ln_top"]), "dot", sigmoid_top=1,
                              loss_function="bce").to(dev())
        m.fuse_qr_interact = fused
        m.emb_update_mode = ops.UPD_DETERMINISTIC
        return m
    on, off = build(True), build(False)
    assert not on._has_qr(on.emb_l)
    X, lS_o, lS_i, target = fixture_batch(0)
    calls = Counted(monkeypatch)
    assert same_bits(predict(on, X, lS_o, lS_i), predict(off, X, lS_o, lS_i))
    assert one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target) == \
        one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (0, 0, 0, 0)
    sa, sb = on.state_dict(), off.state_dict()
    assert all(torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)) for k in sa)
