"""Fused lookup + interaction over quotient-remainder tables of D = 16 / 32 / 64, forward and backward: dlrm_interact_fwd_gather_narrow_qr /
dlrm_interact_bwd_gather_narrow_qr through dlrm_amd.ops, and the model path that DLRM_Net.fuse_qr_interact opens together with
fuse_narrow_interact.

  * op level: R, dx and the gradient buffer of the virtual table list are BIT-IDENTICAL to the two-kernel form (ops.emb_fwd_qr into a feature
    buffer, ops.interact_fwd / ops.interact_bwd over it, ops.emb_qr_bwd_split with the sums that forward saved) — never to the kernels under
    test — and, for in-range ids, to the fp32 narrow fused kernels on tables materialised row by row with the element formula; one test is
    independent of the project's kernels (float64 numpy);
  * model level: both flags on give the prediction bits, the loss and — after one SGD step — the weight_q / weight_r / plain table bits and
    the tower parameters of the flags off.

Batch sizes: a workgroup has four waves and a wave takes one sample per pass, so B = 1 leaves three waves of the only workgroup without a
sample, B = 5 gives the first wave of a second workgroup one sample (every look-ahead of every wave is clamped at B - 1), and B = 300 needs
75 workgroups.  Tables have at most 2000 rows; table 0 has one row, table 3 three.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_narrow_rows as NR
import test_gpu_qr_interact as QI
import test_qr_emb_host as H
from conftest import load_golden, params_with_prefix

pytestmark = pytest.mark.gpu

ROWS = NR.ROWS                                  # 31 tables: F = 32 is the widest shape the kernels take
# 0: a plain table; c = 1: weight_r is a single row; c = 4 > n at tables 0 and 6, c = 7 > n at table 11 (5 rows)
COLL = [4, 0, 3, 1, 7, 0, 4, 3, 0, 7, 1, 7, 0, 3, 7, 4, 0, 1, 3, 0, 7, 4, 3, 0, 1, 7, 4, 0, 3, 7, 1]
BATCHES = NR.BATCHES
SPECIAL = QI.SPECIAL
WIDTHS = (16, 32, 64)
dev, to_dev, same_bits = NR.dev, NR.to_dev, NR.same_bits
n_virtual = QI.n_virtual

assert len(COLL) == len(ROWS) == 31 and {0, 1, 3, 4, 7} == set(COLL) and COLL[11] == 7 > ROWS[11] and COLL[3] == 1 and COLL[:3] == QI.COLL[:3]


_tables = {}


def host_tables(D):
    """(weight_q or plain weight, weight_r or None) per table, uniform in [-1, 1].  Row 0 of table 0's weight_q (QR, c = 4) and of table 1
    (plain) carry -0.0 and subnormals in their first columns; the whole weight_r of table 2 (c = 3) consists of them."""
    if ("host", D) not in _tables:
        rng = np.random.default_rng(2025 + D)
        hs = []
        for t, (n, c) in enumerate(zip(ROWS, COLL)):
            w = rng.uniform(-1.0, 1.0, size=(H.rows_q(n, c) if c else n, D)).astype(np.float32)
            wr = rng.uniform(-1.0, 1.0, size=(c, D)).astype(np.float32) if c else None
            if t in (0, 1):
                w[0, :SPECIAL.size] = SPECIAL
            if t == 2:
                wr[:] = np.tile(SPECIAL, D // SPECIAL.size)[None, :]
            hs.append((w, wr))
        _tables[("host", D)] = hs
    return _tables[("host", D)]


def tables(T, D):
    """device tensors (weights, weights_r) of the first T tables"""
    if ("dev", D) not in _tables:
        hs = host_tables(D)
        _tables[("dev", D)] = ([to_dev(w) for w, _ in hs], [None if r is None else to_dev(r) for _, r in hs])
    W, Wr = _tables[("dev", D)]
    return W[:T], Wr[:T]


def materialised(T, D, op):
    """the [n, D] fp32 table of every category, row by row with the element formula: fmaf(1, Wq[q], +0) op fmaf(1, Wr[r], +0), each rounded
    once (numpy float32 arithmetic is IEEE, subnormals included); fmaf(1, W[id], +0) for a plain table"""
    key = ("mat", D, op)
    if key not in _tables:
        out = []
        zero = np.float32(0.0)
        for (w, wr), n, c in zip(host_tables(D), ROWS, COLL):
            if not c:
                out.append(to_dev(w + zero))
                continue
            q, r, ok = H.qr_split(np.arange(n), n, c)
            assert ok.all() and np.array_equal(q, np.arange(n) // c)
            sq, sr = w[q] + zero, wr[r] + zero
            out.append(to_dev(sq * sr if op == "mult" else sq + sr))
        _tables[key] = out
    return _tables[key][:T]


def pooled(W, Wr, rows, coll, op, bags, B, D, keep=True, pred=None):
    """the [B, T*D] fp32 buffer of the two-kernel form and the sums its forward keeps for the backward (both -7.0-filled first)"""
    from dlrm_amd import ops
    E = torch.full((B, len(W) * D), -7.0, device=dev())
    saved = torch.full((B, 2 * D * sum(1 for c in coll if c)), -7.0, device=dev()) if (keep and op == "mult" and any(coll)) else None
    ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, E, saved, pred=pred)
    return E, saved


def two_kernel_backward(x, E, saved, coll, op, D, m, dR):
    from dlrm_amd import ops
    B, T = x.size(0), len(coll)
    dx, dE = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E), D, m, dR, (dx, dE))
    return dx, ops.emb_qr_bwd_split(coll, op, D, dE, saved)


# ------------------------------------------------------------------------------------------------ 1. the forward grid
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27, 32])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", WIDTHS)
def test_forward_bit_identity_grid(D, F, idx_dtype, op):
    """F = 16 / 17 straddle the NB = 1 / 2 instantiations, F = 32 fills every feature slot"""
    from dlrm_amd import ops
    T = F - 1
    W, Wr = tables(T, D)
    rows, coll = ROWS[:T], COLL[:T]
    rng = np.random.default_rng(F * 10 + D)
    ops.check_index_errors(sync=True)
    for B in BATCHES:
        bags, _ = NR.onehot_bags(rng, rows, B, idx_dtype)
        x = torch.randn((B, D), device=dev())
        E, _ = pooled(W, Wr, rows, coll, op, bags, B, D, keep=False)
        for mode in (0, 1, 2):
            ldr = NR.ldr_of(F, D, mode)
            Wd = ops.interact_out_width(F, D, mode)
            ref = torch.empty((B, ldr), device=dev())
            ops.interact_fwd((x, E), D, mode, ref)
            buf1, R1 = NR.guarded_rows(B, ldr)
            buf2, R2 = NR.guarded_rows(B, ldr)
            ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, mode, R1)
            ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, mode, R2)
            ops.check_index_errors(sync=True)
            what = "B=%d mode=%d" % (B, mode)
            assert not torch.isnan(R1).any(), what
            assert same_bits(R1, ref), what + ": the two-kernel form"
            assert same_bits(R1, R2), what + ": two runs differ"
            assert NR.row_canaries_intact(buf1, buf2), what
            assert bool((R1[:, Wd:] == 0).all()), what + ": padding columns"
            assert same_bits(R1[:, :D], x), what + ": the x block"


# ------------------------------------------------------------------------------------------------ 2. the backward grid
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("F", [2, 3, 16, 17, 27, 32])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", WIDTHS)
def test_backward_bit_identity_grid(D, F, idx_dtype, op):
    """the axes of the forward grid; x, dR, dx, gout are column views of wider allocations (ld = width + 8); with and without INTERACT_RELU_X"""
    from dlrm_amd import ops
    T = F - 1
    W, Wr = tables(T, D)
    rows, coll = ROWS[:T], COLL[:T]
    Tv = n_virtual(coll)
    rng = np.random.default_rng(F * 10 + D + 1)
    ops.check_index_errors(sync=True)
    for B in BATCHES:
        bags, _ = NR.onehot_bags(rng, rows, B, idx_dtype)
        x = NR.wide(NR.x_with_zeros_and_negatives(B, D))
        assert x.stride(0) == D + 8
        E, saved = pooled(W, Wr, rows, coll, op, bags, B, D)
        for mode in (0, 1, 2):
            dR = NR.wide(NR.dR_of(B, F, D, mode))
            for relu in (0, ops.INTERACT_RELU_X):
                m = mode | relu
                dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, D, m, dR)
                outs = []
                for _ in range(2):
                    bx, dx = NR.guarded(B, D)
                    bg, gout = NR.guarded(B, Tv * D)
                    ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, m, dR, dx, gout)
                    outs.append((bx, dx, bg, gout))
                ops.check_index_errors(sync=True)
                (bx, dx, bg, gout), (bx2, dx2, bg2, gout2) = outs
                what = "B=%d mode=%d relu=%d" % (B, mode, relu)
                assert not torch.isnan(dx).any() and not torch.isnan(gout).any(), what
                assert same_bits(dx, dx_ref) and same_bits(gout, g_ref), what + ": the two-kernel form"
                assert same_bits(dx, dx2) and same_bits(gout, gout2), what + ": two runs differ"
                assert NR.canaries_intact(bx, bg, bx2, bg2), what
                if relu:
                    assert bool((dx[x <= 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------ 3. against the fp32 narrow kernels
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("F", [17, 32])
@pytest.mark.parametrize("D", WIDTHS)
def test_equals_the_fp32_narrow_kernels_on_materialised_tables(D, F, op):
    """for in-range ids the composed row IS a row of the table materialised with the element formula: R and dx have the bits of
    interact_{fwd,bwd}_gather_narrow over those tables"""
    from dlrm_amd import ops
    T, B = F - 1, 300
    W, Wr = tables(T, D)
    rows, coll = ROWS[:T], COLL[:T]
    mat = materialised(T, D, op)
    bags, _ = NR.onehot_bags(np.random.default_rng(F + D), rows, B)
    x = NR.x_with_zeros_and_negatives(B, D)
    ops.check_index_errors(sync=True)
    for mode in (0, 1, 2):
        ldr = NR.ldr_of(F, D, mode)
        R, R32 = torch.empty((B, ldr), device=dev()), torch.empty((B, ldr), device=dev())
        ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, mode, R)
        ops.interact_fwd_gather_narrow(x, mat, bags, D, mode, R32)
        assert same_bits(R, R32), mode
        dR = NR.dR_of(B, F, D, mode)
        dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, n_virtual(coll) * D), device=dev())
        dx32, dE32 = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
        ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, mode, dR, dx, gout)
        ops.interact_bwd_gather_narrow(x, mat, bags, D, mode, dR, dx32, dE32)
        assert same_bits(dx, dx32), mode
        if op == "add":                 # every slot of an ADD call is the gradient row itself
            v = 0
            for t, c in enumerate(coll):
                for _ in range(2 if c else 1):
                    assert same_bits(gout[:, v * D:(v + 1) * D], dE32[:, t * D:(t + 1) * D]), (mode, t)
                    v += 1
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 4. independent of the project's kernels
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("D", WIDTHS)
def test_against_float64_numpy(D, op):
    """R, dx and gout against float64 numpy on the composed fp32 elements, within the any-order fp32 summation bounds of
    tests/test_gpu_narrow_interact.py::test_against_float64_numpy (u = 2^-24):
    forward pair (a, b): |err| <= (D + 1) u sum_k |a_k| |b_k|;  backward: |err| <= bnd = (F + 2) u (sum_j |S_ij| |T_jd| + |dR_d|), the dR_d term
    for feature 0 only.  A gout slot that is a product dT * s, s an exact fp32 table value, is one more rounding of a value within bnd of dT:
    |fl(g s) - dT64 s| <= (1 + u) bnd |s| + u |dT64 s|.  ADD slots and plain slots are the gradient row: within bnd.
    Table values have |v| in [0.25, 1]: nothing underflows, and a composed element is one exactly rounded fp32 operation of them."""
    from dlrm_amd import ops
    B, F = 64, 27
    T = F - 1
    rows, coll = ROWS[:T], COLL[:T]
    Tv = n_virtual(coll)
    rng = np.random.default_rng(303 + D)

    def values(shape):
        return (rng.uniform(0.25, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    hs = [(values((H.rows_q(n, c) if c else n, D)), values((c, D)) if c else None) for n, c in zip(rows, coll)]
    W, Wr = [to_dev(w) for w, _ in hs], [None if r is None else to_dev(r) for _, r in hs]
    bags, idx = NR.onehot_bags(np.random.default_rng(33), rows, B)
    xn = rng.standard_normal((B, D)).astype(np.float32)
    x = to_dev(xn)
    Wd = ops.interact_out_width(F, D, 0)
    ldr = NR.ldr_of(F, D, 0)
    dRn = rng.standard_normal((B, Wd)).astype(np.float32)
    dR = torch.zeros((B, ldr), device=dev())
    dR[:, :Wd] = to_dev(dRn)
    R = torch.empty((B, ldr), device=dev())
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, Tv * D), device=dev())
    ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, R)
    ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout)
    ops.check_index_errors(sync=True)
    # the composed fp32 elements (numpy float32 arithmetic is IEEE: one rounding), then everything in float64
    feat = np.empty((B, F, D), dtype=np.float64)
    feat[:, 0] = xn
    comps = []
    for t, ((w, wr), c) in enumerate(zip(hs, coll)):
        if c:
            sq, sr = w[idx[t] // c], wr[idx[t] % c]
            feat[:, 1 + t] = sq * sr if op == "mult" else sq + sr
            comps.append((sq.astype(np.float64), sr.astype(np.float64)))
        else:
            feat[:, 1 + t] = w[idx[t]]
            comps.append(None)
    u = 2.0 ** -24
    li, lj = np.tril_indices(F, -1)
    Z = np.einsum("bik,bjk->bij", feat, feat)
    Zabs = np.einsum("bik,bjk->bij", np.abs(feat), np.abs(feat))
    got = R.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[:, :D], xn.astype(np.float64))
    assert (got[:, Wd:] == 0).all()
    err_f = np.abs(got[:, D:Wd] - Z[:, li, lj])
    bound_f = (D + 1) * u * Zabs[:, li, lj]
    S = np.zeros((B, F, F))
    S[:, li, lj] = dRn[:, D:].astype(np.float64)
    S[:, lj, li] = dRn[:, D:].astype(np.float64)
    dT = np.einsum("bij,bjd->bid", S, feat)
    dTabs = np.einsum("bij,bjd->bid", np.abs(S), np.abs(feat))
    dT[:, 0] += dRn[:, :D]
    dTabs[:, 0] += np.abs(dRn[:, :D])
    bnd = (F + 2) * u * dTabs
    err_x = np.abs(dx.cpu().numpy().astype(np.float64) - dT[:, 0])
    gg = gout.cpu().numpy().astype(np.float64)
    want_g, bound_g = [], []
    for t, cs in enumerate(comps):
        g, b = dT[:, 1 + t], bnd[:, 1 + t]
        if cs is None:
            want_g.append(g); bound_g.append(b)
        elif op == "add":
            want_g += [g, g]; bound_g += [b, b]
        else:
            for s in (cs[1], cs[0]):                  # the q slot gets dout * sr, the r slot dout * sq
                want_g.append(g * s)
                bound_g.append((1 + u) * b * np.abs(s) + u * np.abs(g * s))
    want_g, bound_g = np.concatenate(want_g, axis=1), np.concatenate(bound_g, axis=1)
    err_g = np.abs(gg - want_g)
    print("worst error / bound: forward %.3g, dx %.3g, gout %.3g" % (float((err_f / np.maximum(bound_f, 1e-300)).max()),
          float((err_x / np.maximum(bnd[:, 0], 1e-300)).max()), float((err_g / np.maximum(bound_g, 1e-300)).max())))
    assert (err_f <= bound_f).all()
    assert (err_x <= bnd[:, 0]).all()
    assert (err_g <= bound_g).all()


# ------------------------------------------------------------------------------------------------ 5. the float32 quotient above 2^24, rows beyond 4 GiB
BIG_C = 4
BIG_N = BIG_C * (2 ** 24 + 4096)          # weight_q: 16,781,312 rows of 256 bytes = 4 GiB + 1 MiB, never filled as a whole


@pytest.mark.parametrize("op", ["mult", "add"])
def test_large_table_float32_quotient_and_rows_beyond_4_gib(op):
    """D = 64.  Half of the ids from [2^24, 2^26) and half from [2^26, n): float32 quotients that are not id // 4, weight_q rows at byte
    offsets that do not fit 32 bits, and the few ids at the top of the table whose float32 quotient is ceil(n / c): no row — refused and
    reported.  Only the weight_q rows the lookups name are written, from a small table."""
    from dlrm_amd import ops
    D, B = 64, 1000
    nq = H.rows_q(BIG_N, BIG_C)
    assert nq == 16_781_312 and nq * 4 * D == 2 ** 32 + 2 ** 20
    rng = np.random.default_rng(44)
    ids = np.where(np.arange(B) % 2 == 0, rng.integers(2 ** 24, 2 ** 26, size=B), rng.integers(2 ** 26, BIG_N, size=B)).astype(np.int64)
    ids[0], ids[1], ids[-1] = BIG_N - 2, 0, BIG_N - 1
    q, r, ok = H.qr_split(ids, BIG_N, BIG_C)
    assert np.array_equal(q, (torch.from_numpy(ids) / BIG_C).long().numpy())
    n_diff, n_far, n_refused = int((q[ok] != ids[ok] // BIG_C).sum()), int((q[ok] * 4 * D >= 2 ** 32).sum()), int((~ok).sum())
    print("float32 quotient != id // c: %d, accepted rows beyond 4 GiB: %d, refused: %d" % (n_diff, n_far, n_refused))
    assert n_diff >= B // 16                       # the test can tell the two mappings apart
    assert n_far >= B // 4
    assert 1 <= n_refused <= 8 and not ok[-1] and q[-1] == nq
    refused = "|".join(str(int(i)) for i in ids[~ok])
    want_msg = r"index (%s), rows %d" % (refused, BIG_N)
    uniq = np.unique(q[ok])
    small = torch.rand((uniq.size, D), device=dev()) - 0.5
    wr = torch.rand((BIG_C, D), device=dev()) - 0.5
    rows, coll = [BIG_N], [BIG_C]
    big = torch.empty((nq, D), device=dev())
    try:
        big.index_copy_(0, to_dev(uniq), small)
        ops.check_index_errors(sync=True)
        for idx_dtype in (torch.int64, torch.int32):
            bags = ops.BagBatch([torch.arange(B, device=dev(), dtype=idx_dtype)], [to_dev(ids, idx_dtype)])
            x = NR.x_with_zeros_and_negatives(B, D)
            ldr = NR.ldr_of(2, D, 0)
            E, saved = pooled([big], [wr], rows, coll, op, bags, B, D)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            # the rows really are the float-quotient rows of the small table; a refused lookup gives the zero row
            okd, zeros = to_dev(ok)[:, None], torch.zeros((B, D), device=dev())
            sq = torch.where(okd, small[to_dev(np.searchsorted(uniq, np.where(ok, q, uniq[0])))] + 0.0, zeros)
            sr = torch.where(okd, wr[to_dev(np.where(ok, r, 0))] + 0.0, zeros)
            assert same_bits(E, sq * sr if op == "mult" else sq + sr)
            ref, R = torch.empty((B, ldr), device=dev()), torch.full((B, ldr), float("nan"), device=dev())
            ops.interact_fwd((x, E), D, 0, ref)
            dR = NR.dR_of(B, 2, D, 0)
            dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, D, 0, dR)
            ops.interact_fwd_gather_narrow_qr(x, [big], [wr], rows, coll, op, bags, D, 0, R)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            dx, gout = torch.full((B, D), float("nan"), device=dev()), torch.full((B, 2 * D), float("nan"), device=dev())
            ops.interact_bwd_gather_narrow_qr(x, [big], [wr], rows, coll, op, bags, D, 0, dR, dx, gout)
            with pytest.raises(IndexError, match=want_msg):
                ops.check_index_errors(sync=True)
            assert same_bits(R, ref)
            assert same_bits(dx, dx_ref) and same_bits(gout, g_ref)
    finally:
        del big
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 6. bad input
TOP_N, TOP_C = 18_750_000, 4          # id n - 1 rounds to n in float32: its quotient ceil(n / c) is no row of weight_q


@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("D", [16, 64])
def test_out_of_range_ids_are_reported_and_give_the_zero_row(D, idx_dtype, op):
    """ids that are negative, equal to n, very large, and an id < n whose float32 quotient is no row (table 3: 18,750,000 categories, of which
    only weight_q rows 0 .. 127 are written and looked up otherwise): reported, the zero row, gout rows as the two-kernel form writes them;
    every other sample has the bits of a clean run"""
    from dlrm_amd import ops
    B, F = 50, 5
    W3, Wr3 = tables(3, D)
    rows, coll = ROWS[:3] + [TOP_N], COLL[:3] + [TOP_C]             # QR (c = 4, n = 1), plain, QR (c = 3), QR (c = 4)
    Tv = n_virtual(coll)
    q_top, _, ok_top = H.qr_split(np.array([TOP_N - 1]), TOP_N, TOP_C)
    assert not ok_top[0] and q_top[0] == H.rows_q(TOP_N, TOP_C)
    rng = np.random.default_rng(5)
    clean = [rng.integers(0, n, size=B).astype(np.int64) for n in rows[:3]] + [rng.integers(0, 512, size=B).astype(np.int64)]
    idx = [c.copy() for c in clean]
    idx[0][9] = rows[0]                # == n of a QR table: its quotient 0 IS a row of weight_q, the id is still no category
    idx[1][7] = rows[1] + 3            # too large, plain table
    idx[2][31] = -1                    # negative, QR table
    idx[2][40] = rows[2]               # == n
    idx[0][44] = 2 ** 31 - 1 if idx_dtype == torch.int32 else 2 ** 40 + 5      # very large
    idx[3][22] = TOP_N - 1             # < n, its quotient is no row
    bad = [9, 7, 31, 40, 44, 22]
    good = [b for b in range(B) if b not in bad]
    offs = [torch.arange(B, device=dev(), dtype=idx_dtype) for _ in rows]
    top = torch.empty((H.rows_q(TOP_N, TOP_C), D), device=dev())
    try:
        top[:128] = torch.rand((128, D), device=dev()) - 0.5
        W, Wr = list(W3) + [top], list(Wr3) + [torch.rand((TOP_C, D), device=dev()) - 0.5]

        def bags(ids):
            return ops.BagBatch(offs, [to_dev(i, idx_dtype) for i in ids])
        x = NR.x_with_zeros_and_negatives(B, D)
        x[:, 0] = 1.0
        ldr = NR.ldr_of(F, D, 0)
        dR = NR.dR_of(B, F, D, 0)
        ops.check_index_errors(sync=True)
        # the two-kernel form: its lookup reports the same ids
        E, saved = pooled(W, Wr, rows, coll, op, bags(idx), B, D)
        with pytest.raises(IndexError, match="out of range"):
            ops.check_index_errors(sync=True)
        assert bool((E[9, :D].view(torch.int32) == 0).all()) and bool((E[22, 3 * D:].view(torch.int32) == 0).all())
        ref = torch.empty((B, ldr), device=dev())
        ops.interact_fwd((x, E), D, 0, ref)
        dx_ref, g_ref = two_kernel_backward(x, E, saved, coll, op, D, 0, dR)
        E_c, saved_c = pooled(W, Wr, rows, coll, op, bags(clean), B, D)
        ref_c = torch.empty((B, ldr), device=dev())
        ops.interact_fwd((x, E_c), D, 0, ref_c)
        dx_c, g_c = two_kernel_backward(x, E_c, saved_c, coll, op, D, 0, dR)
        ops.check_index_errors(sync=True)
        # forward
        R = torch.full((B, ldr), float("nan"), device=dev())
        ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags(idx), D, 0, R)
        with pytest.raises(IndexError, match=r"index (1|40|-1|2000|2147483647|1099511627781|18749999), rows (1|37|2000|18750000) "):
            ops.check_index_errors(sync=True)
        assert same_bits(R, ref)
        assert same_bits(R[good], ref_c[good])
        # pairs (1, 0), (2, 0), (3, 0), (4, 0) of the bad samples: x . zero row = +0.0
        zero_bits = R[[9, 44, 7, 31, 40, 22], [D + 0, D + 0, D + 1, D + 3, D + 3, D + 6]].view(torch.int32)
        assert bool((zero_bits == 0).all())
        ops.check_index_errors(sync=True)            # reported once
        # backward: gout as the two-kernel form writes it (dout * (+0) for "mult", dout for "add", a copy for the plain table)
        dx, gout = torch.full((B, D), float("nan"), device=dev()), torch.full((B, Tv * D), float("nan"), device=dev())
        ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags(idx), D, 0, dR, dx, gout)
        with pytest.raises(IndexError, match="out of range"):
            ops.check_index_errors(sync=True)
        assert not torch.isnan(dx).any() and not torch.isnan(gout).any()
        assert same_bits(dx, dx_ref) and same_bits(gout, g_ref)
        assert same_bits(dx[good], dx_c[good]) and same_bits(gout[good], g_c[good])
        ops.check_index_errors(sync=True)
    finally:
        del top
        torch.cuda.empty_cache()


@pytest.mark.parametrize("D", [16, 64])
def test_broken_bag_start_is_reported(D):
    from dlrm_amd import ops
    B = 40
    W, Wr = tables(2, D)
    rows, coll = ROWS[:2], COLL[:2]
    rng = np.random.default_rng(6)
    off = np.arange(B, dtype=np.int64)
    off[11] = 10                      # bag 10 has two lookups, bag 11 none: nnz == B, not one lookup per bag
    bags = ops.BagBatch([to_dev(off), torch.arange(B, device=dev())], [to_dev(rng.integers(0, n, size=B).astype(np.int64)) for n in rows])
    x = torch.randn((B, D), device=dev())
    R = torch.empty((B, NR.ldr_of(3, D, 0)), device=dev())
    ops.check_index_errors(sync=True)
    ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, "mult", bags, D, 0, R)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, "mult", bags, D, 0, NR.dR_of(B, 3, D, 0), dx, gout)
    with pytest.raises(IndexError, match="does not start at its own position"):
        ops.check_index_errors(sync=True)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 7. launch predicates
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("D", [16, 64])
def test_launch_predicates(D, op):
    """with (flag, 0) / (flag, 1) exactly one of the fused form and the two-kernel form writes: the launches that must not run — the
    in-place multiplication behind the fused MULT backward included — leave their -7.0-filled outputs untouched, the other form gives the
    unpredicated bits"""
    from dlrm_amd import ops
    B, F = 70, 6
    T = F - 1
    W, Wr = tables(T, D)
    rows, coll = ROWS[:T], COLL[:T]
    Tv, nq = n_virtual(coll), sum(1 for c in coll if c)
    bags, _ = NR.onehot_bags(np.random.default_rng(8), rows, B)
    x = NR.x_with_zeros_and_negatives(B, D)
    ldr = NR.ldr_of(F, D, 0)
    dR = NR.dR_of(B, F, D, 0)
    E_ref = torch.empty((B, T * D), device=dev())
    sv_ref = torch.empty((B, 2 * nq * D), device=dev())
    ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, E_ref, sv_ref)
    ref = torch.empty((B, ldr), device=dev())
    ops.interact_fwd((x, E_ref), D, 0, ref)
    dx_ref, dE_ref = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd((x, E_ref), D, 0, dR, (dx_ref, dE_ref))
    g_ref = ops.emb_qr_bwd_split(coll, op, D, dE_ref, sv_ref)
    zero, one = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(1, dtype=torch.int32, device=dev())

    def filled(*shape):
        return torch.full(shape, -7.0, device=dev())

    def untouched(*ts):
        return all(bool((t == -7.0).all()) for t in ts)
    for flag in (zero, one):
        fused_runs = flag is zero                      # the fused form goes behind (flag, 0), the two-kernel form behind (flag, 1)
        R, dx, gout = filled(B, ldr), filled(B, D), filled(B, Tv * D)
        ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, R, pred=(flag, 0))
        ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout, pred=(flag, 0))
        E2, sv2 = filled(B, T * D), filled(B, 2 * nq * D)
        ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, E2, sv2, pred=(flag, 1))
        R2, dx2, dE2, g2 = filled(B, ldr), filled(B, D), filled(B, T * D), filled(B, Tv * D)
        ops.interact_fwd((x, E_ref), D, 0, R2, pred=(flag, 1))
        ops.interact_bwd((x, E_ref), D, 0, dR, (dx2, dE2), pred=(flag, 1))
        ops.emb_qr_bwd_split(coll, op, D, dE_ref, sv_ref, g2, pred=(flag, 1))
        ops.check_index_errors(sync=True)
        if fused_runs:
            assert same_bits(R, ref) and same_bits(dx, dx_ref) and same_bits(gout, g_ref)
            assert untouched(E2, R2, dx2, dE2, g2) and (op == "add" or untouched(sv2))
        else:
            assert untouched(R, dx, gout)
            assert same_bits(E2, E_ref) and same_bits(R2, ref) and same_bits(dx2, dx_ref) and same_bits(dE2, dE_ref) and same_bits(g2, g_ref)
            assert op == "add" or same_bits(sv2, sv_ref)
    # ... and the opposite sense of both
    R, dx, gout = filled(B, ldr), filled(B, D), filled(B, Tv * D)
    ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, R, pred=(one, 1))
    ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout, pred=(one, 1))
    assert same_bits(R, ref) and same_bits(dx, dx_ref) and same_bits(gout, g_ref)
    R, dx, gout = filled(B, ldr), filled(B, D), filled(B, Tv * D)
    ops.interact_fwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, R, pred=(zero, 1))
    ops.interact_bwd_gather_narrow_qr(x, W, Wr, rows, coll, op, bags, D, 0, dR, dx, gout, pred=(zero, 1))
    assert untouched(R, dx, gout)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 8. refusals
E_ARG, E_RANGE, E_MODE = QI.E_ARG, QI.E_RANGE, QI.E_MODE


def raw_call(which, x, W, Wr, rows, coll, op_code, bags, mode, R_or_dR, dx=None, gout=None, d=16):
    """the C entry point itself, with operands ops.* would refuse first (an unknown op, a null weight_r)"""
    from dlrm_amd import _lib, ops
    lib = _lib.load()
    T = len(W)
    wp = _lib.ptr_array([w.data_ptr() for w in W])
    wrp = _lib.ptr_array([0 if r is None else r.data_ptr() for r in Wr])
    common = (x.size(0), 1 + T, d, C.c_void_p(x.data_ptr()), ops._ld(x), wp, wrp, _lib.i64_array(rows),
              (C.c_int * T)(*coll), op_code, bags._idx, bags._off, bags.idx_bits, mode, C.c_void_p(R_or_dR.data_ptr()), ops._ld(R_or_dR))
    st = ops._stream(x)
    if which == "fwd":
        return lib.dlrm_interact_fwd_gather_narrow_qr(*common, None, None, 0, st)
    return lib.dlrm_interact_bwd_gather_narrow_qr(*common, C.c_void_p(dx.data_ptr()), ops._ld(dx), C.c_void_p(gout.data_ptr()), ops._ld(gout),
                                                  None, None, 0, st)


def test_refused_operands():
    from dlrm_amd import ops
    B, D = 8, 16
    assert ops.gather_narrow_qr_ok(32, 16) and ops.gather_narrow_qr_ok(2, 64) and ops.gather_narrow_qr_ok(27, 32)
    assert not ops.gather_narrow_qr_ok(2, 128) and not ops.gather_narrow_qr_ok(2, 48) and not ops.gather_narrow_qr_ok(33, 16)
    g = torch.Generator(device=dev()).manual_seed(1)
    wq, wr = torch.rand((25, D), device=dev(), generator=g), torch.rand((4, D), device=dev(), generator=g)
    wp = torch.rand((100, D), device=dev(), generator=g)
    rows, coll = [100, 100], [4, 0]
    bags = ops.BagBatch([torch.arange(B, device=dev())] * 2, [torch.arange(B, device=dev()) * 3] * 2)
    x, R = torch.randn((B, D), device=dev()), torch.empty((B, NR.ldr_of(3, D, 0)), device=dev())
    dR = NR.dR_of(B, 3, D, 0)
    dx, gout = torch.empty((B, D), device=dev()), torch.empty((B, 3 * D), device=dev())
    ops.interact_fwd_gather_narrow_qr(x, [wq, wp], [wr, None], rows, coll, "mult", bags, D, 0, R)                       # (the operands are fine as they stand)
    ops.interact_bwd_gather_narrow_qr(x, [wq, wp], [wr, None], rows, coll, "mult", bags, D, 0, dR, dx, gout)
    assert raw_call("fwd", x, [wq, wp], [wr, None], rows, coll, 0, bags, 0, R) == 0
    assert raw_call("bwd", x, [wq, wp], [wr, None], rows, coll, 1, bags, 0, dR, torch.empty_like(dx), torch.empty_like(gout)) == 0      # (ADD)
    ops.check_index_errors(sync=True)

    def both(match, x_=x, W=(wq, wp), Wr_=(wr, None), R_=R, dR_=dR, dx_=dx, gout_=gout, bags_=bags, d=D):
        with pytest.raises(RuntimeError, match=match):
            ops.interact_fwd_gather_narrow_qr(x_, list(W), list(Wr_), rows, coll, "mult", bags_, d, 0, R_)
        with pytest.raises(RuntimeError, match=match):
            ops.interact_bwd_gather_narrow_qr(x_, list(W), list(Wr_), rows, coll, "add", bags_, d, 0, dR_, dx_, gout_)
    # D = 128 and D = 48
    for d in (128, 48):
        z = lambda n: torch.zeros((n, d), device=dev())       # noqa: E731
        both("DLRM_E_MODE", x_=z(B), W=(z(25), z(100)), Wr_=(z(4), None), R_=torch.empty((B, d + 4), device=dev()),
             dR_=torch.zeros((B, d + 4), device=dev()), dx_=z(B), gout_=torch.empty((B, 3 * d), device=dev()), d=d)
    # the D = 128 QR kernels keep refusing D = 16
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.interact_fwd_gather_qr(x, [wq, wp], [wr, None], rows, coll, "mult", bags, D, 0, R.clone())
    # a weight_q / weight_r / plain table 4 or 8 bytes off 16-byte alignment; 16 bytes off is fine and gives the same bits
    for nbytes in (4, 8):
        assert not ops.qr_tables_aligned([NR.offset_view(wq, nbytes)], [wr]) and not ops.qr_tables_aligned([wq], [NR.offset_view(wr, nbytes)])
        both("DLRM_E_MODE", W=(NR.offset_view(wq, nbytes), wp))
        both("DLRM_E_MODE", Wr_=(NR.offset_view(wr, nbytes), None))
        both("DLRM_E_MODE", W=(wq, NR.offset_view(wp, nbytes)))
    R16, dx16, gout16 = torch.empty_like(R), torch.empty_like(dx), torch.empty_like(gout)
    W16, Wr16 = [NR.offset_view(wq, 16), NR.offset_view(wp, 16)], [NR.offset_view(wr, 16), None]
    ops.interact_fwd_gather_narrow_qr(x, W16, Wr16, rows, coll, "mult", bags, D, 0, R16)
    ops.interact_bwd_gather_narrow_qr(x, W16, Wr16, rows, coll, "mult", bags, D, 0, dR, dx16, gout16)
    assert same_bits(R16, R) and same_bits(dx16, dx) and same_bits(gout16, gout)
    # a bf16 table
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        ops.interact_fwd_gather_narrow_qr(x, [wq.to(torch.bfloat16), wp], [wr, None], rows, coll, "mult", bags, D, 0, R.clone())
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        ops.interact_bwd_gather_narrow_qr(x, [wq, wp.to(torch.bfloat16)], [wr, None], rows, coll, "mult", bags, D, 0, dR, dx.clone(), gout.clone())
    # an unknown op, a null weight_r for a QR table, collisions < 0, rows <= 0: DLRM_E_ARG (ops refuses them itself: the C call)
    with pytest.raises(RuntimeError, match="'mult' or 'add'"):
        ops.interact_fwd_gather_narrow_qr(x, [wq, wp], [wr, None], rows, coll, "concat", bags, D, 0, R.clone())
    assert raw_call("fwd", x, [wq, wp], [wr, None], rows, coll, 2, bags, 0, R) == E_ARG
    assert raw_call("bwd", x, [wq, wp], [wr, None], rows, coll, -1, bags, 0, dR, dx, gout) == E_ARG
    assert raw_call("fwd", x, [wq, wp], [None, None], rows, coll, 0, bags, 0, R) == E_ARG
    assert raw_call("bwd", x, [wq, wp], [None, None], rows, coll, 0, bags, 0, dR, dx, gout) == E_ARG
    assert raw_call("fwd", x, [wq, wp], [wr, None], rows, [-1, 0], 0, bags, 0, R) == E_ARG
    assert raw_call("fwd", x, [wq, wp], [wr, None], [0, 100], coll, 0, bags, 0, R) == E_ARG
    # more than 0xFFFFFFFF rows of weight_q / of a plain table (nothing is launched: the pointers are never followed)
    assert raw_call("fwd", x, [wq, wp], [wr, None], [4 * 0xFFFFFFFF + 1, 100], coll, 0, bags, 0, R) == E_RANGE
    assert raw_call("bwd", x, [wq, wp], [wr, None], [100, 0x100000000], coll, 0, bags, 0, dR, dx, gout) == E_RANGE
    # a gout narrower than the virtual table list: ops refuses the tensor, the C call the leading dimension
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.interact_bwd_gather_narrow_qr(x, [wq, wp], [wr, None], rows, coll, "mult", bags, D, 0, dR, dx, gout[:, :2 * D])
    assert raw_call("bwd", x, [wq, wp], [wr, None], rows, coll, 0, bags, 0, dR, dx, torch.empty((B, 2 * D), device=dev())) == E_ARG
    # per-sample weights, nnz != B
    ones = torch.ones(B, device=dev())
    wbags = ops.BagBatch([torch.arange(B, device=dev())] * 2, [torch.zeros(B, dtype=torch.int64, device=dev())] * 2, [ones, ones])
    both("per-sample weights", bags_=wbags)
    mbags = ops.BagBatch([torch.arange(B, device=dev()) * 2] * 2, [torch.zeros(2 * B, dtype=torch.int64, device=dev())] * 2)
    both("exactly one lookup per bag", bags_=mbags)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------------ 9. the models
D64_LN_EMB = [1460, 24, 583]            # threshold 200: QR, plain, QR
NAMES = ("interact_fwd_gather_narrow_qr", "interact_bwd_gather_narrow_qr", "emb_fwd_qr", "emb_qr_bwd_split", "interact_fwd", "interact_bwd",
         "interact_fwd_gather_qr", "interact_bwd_gather_qr")
CFGS = ["d16_mult", "d16_add", "d64_mult", "d64_add"]


def ln_emb_of(cfg):
    return load_golden("qr_training")[1]["cases"][cfg[4:]]["ln_emb"] if cfg.startswith("d16") else D64_LN_EMB


def qr_model(cfg, narrow, qr, mode=None, **kw):
    """d16_*: the `mult` / `add` models of tests/golden/qr_training.npz from their stored start parameters; d64_*: a seeded 3-table model"""
    import dlrm_amd
    op = cfg[4:]
    if cfg.startswith("d16"):
        d, meta = load_golden("qr_training")
        m = H.build_qr_model(meta["cases"][op], meta["qr_threshold"], params=params_with_prefix(d, op + ".start"), seed=1, **kw)
    else:
        np.random.seed(3)
        torch.manual_seed(3)
        m = dlrm_amd.DLRM_Net(64, np.asarray(D64_LN_EMB), np.asarray([13, 32, 64]), np.asarray([64 + 6, 32, 1]), "dot", sigmoid_top=1,
                              loss_function="bce", qr_flag=True, qr_operation=op, qr_collisions=4, qr_threshold=200, **kw)
    m = m.to(dev())
    m.fuse_narrow_interact, m.fuse_qr_interact = narrow, qr
    if mode is not None:
        m.emb_update_mode = mode
    return m


def batch(cfg, seed, B=64, state="tagged", hots=1, distinct=False):
    """one-hot batches made here (the fixture's own batches are multi-hot).  distinct: B = 3 and no table row — of a plain table, of a
    weight_q or of a weight_r — is named twice (ids 0, c + 1, 2 c + 2 have the quotients and the remainders 0, 1, 2 for c >= 3)"""
    from dlrm_amd import ops
    ln_emb = ln_emb_of(cfg)
    rng = np.random.default_rng(seed)
    if distinct:
        B = 3
        assert hots == 1 and min(ln_emb) >= 3
    X = to_dev(rng.random((B, 13)).astype(np.float32))
    lS_o = [torch.arange(B, device=dev()) * hots for _ in ln_emb]
    if distinct:
        c = 7 if cfg == "d16_add" else 4                # (tables of more than 200 rows are the QR tables)
        lS_i = [to_dev(np.array([0, 1, 2] if n <= 200 else [0, c + 1, 2 * c + 2], dtype=np.int64)) for n in ln_emb]
    else:
        lS_i = [to_dev(rng.integers(0, n, size=B * hots).astype(np.int64)) for n in ln_emb]
    target = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    if state == "tagged":
        for o in lS_o:
            ops.mark_one_lookup_per_bag(o)
    if state == "ragged":
        lS_o[2][17] = 16                # bag 16 has two lookups, bag 17 none: nnz == B, not one lookup per bag
    return X, lS_o, lS_i, target


def counted(monkeypatch):
    return NR.Counted(monkeypatch, NAMES)


predict, one_step, update_mode = QI.predict, QI.one_step, QI.update_mode


def same_parameters(a, b):
    QI.same_parameters(a, b)


@pytest.mark.parametrize("mode_name", QI.UPDATE_MODES)
@pytest.mark.parametrize("cfg", CFGS)
def test_model_takes_the_fused_kernels_and_gives_the_bits_of_the_two_kernel_form(cfg, mode_name, monkeypatch):
    """Both models hand the same gradient bits to the same update kernel, so every parameter is compared bit for bit in all three modes.
    Sorted and deterministic: a batch of 64 with many lookups of the same row.  Atomic: include/dlrm_hip.h leaves the order in which the
    gradients of lookups of the SAME row are accumulated unspecified (LDS and global fp32 atomics), so the bits of such a step are not a
    function of its inputs — two steps of the flags-off model alone may differ; its batch names every table row at most once (B = 3), which
    makes the step's result order-free and the comparison exact."""
    mode = update_mode(mode_name)
    on, off = qr_model(cfg, True, True, mode), qr_model(cfg, False, False, mode)
    X, lS_o, lS_i, target = batch(cfg, 21, distinct=mode_name == "atomic")
    if mode_name == "atomic":
        for n, c, i in zip(ln_emb_of(cfg), on._qr_spec(on.emb_l)[1], lS_i):
            i = i.cpu().numpy()
            assert (np.unique(i // c).size == 3 and np.unique(i % c).size == 3) if c else np.unique(i).size == 3, n
    want = predict(off, X, lS_o, lS_i)
    calls = counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert calls.counts() == (1, 0, 0, 0, 0, 0, 0, 0) and calls.preds["interact_fwd_gather_narrow_qr"] == [None]
    assert same_bits(got, want)
    before = {k: v.clone() for k, v in on.state_dict().items()}
    l_on = one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (2, 1, 0, 0, 0, 0, 0, 0) and calls.preds["interact_bwd_gather_narrow_qr"] == [None]
    l_off = one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (2, 1, 1, 1, 1, 1, 0, 0)                  # (the off-model's two-kernel form)
    assert l_on == l_off
    same_parameters(on, off)
    after = on.state_dict()
    assert all(not torch.equal(before[k], after[k]) for k in after if k.endswith("weight_q") or k.endswith("weight_r"))   # (the step moved the tables)


@pytest.mark.parametrize("state", ["fresh", "ragged"])
@pytest.mark.parametrize("cfg", CFGS)
def test_other_offsets_states_give_the_bits_of_the_two_kernel_form(cfg, state, monkeypatch):
    """fresh: offsets nobody vouched for -> the device-flag path: the fused kernels behind (flag, 0), the two-kernel form behind (flag, 1),
    forward and backward, no host wait.  ragged: nnz == B with an empty bag next to a two-lookup bag -> the flag path runs the two-kernel
    form."""
    from dlrm_amd import ops
    on, off = qr_model(cfg, True, True, ops.UPD_DETERMINISTIC), qr_model(cfg, False, False, ops.UPD_DETERMINISTIC)
    X, lS_o, lS_i, target = batch(cfg, 22, state=state)
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    lS_o = [o.clone() for o in lS_o]                  # fresh tensor objects: no verdict is cached for them
    calls = counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert same_bits(got, want)
    assert calls.counts() == (1, 0, 1, 0, 1, 0, 0, 0)
    assert calls.preds["interact_fwd_gather_narrow_qr"][0][1] == 0 and calls.preds["emb_fwd_qr"][0][1] == 1 and calls.preds["interact_fwd"][0][1] == 1
    lS_o = [o.clone() for o in lS_o]
    l_on = one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (2, 1, 2, 1, 2, 1, 0, 0)
    assert calls.preds["interact_bwd_gather_narrow_qr"][0][1] == 0 and calls.preds["interact_bwd"][0][1] == 1
    assert calls.preds["emb_qr_bwd_split"][0][1] == 1
    assert l_on == l_off
    same_parameters(on, off)


@pytest.mark.parametrize("flags", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("cfg", ["d16_mult", "d64_add"])
def test_with_either_flag_off_the_new_ops_are_never_called(cfg, flags, monkeypatch):
    m = qr_model(cfg, *flags)
    X, lS_o, lS_i, target = batch(cfg, 5)
    calls = counted(monkeypatch)
    predict(m, X, lS_o, lS_i)
    assert calls.counts() == (0, 0, 1, 0, 1, 0, 0, 0)
    one_step(m, torch.optim.SGD(m.parameters(), lr=0.1), X, lS_o, lS_i, target)
    assert calls.counts() == (0, 0, 2, 1, 2, 1, 0, 0)


@pytest.mark.parametrize("case", ["multihot", "cat", "md"])
def test_other_models_keep_the_two_kernel_form(case, monkeypatch):
    import dlrm_amd
    from dlrm_amd import ops
    cfg, B, hots = "d16_mult", 48, 3 if case == "multihot" else 1
    if case == "md":
        import test_md_emb_host as MH
        d, meta = load_golden("md_training")
        mcase = meta["cases"]["pow2"]              # base dimension 16

        def build(flag):
            m = MH.build_md_model(mcase, meta["md_threshold"], seed=1).to(dev())
            m.fuse_narrow_interact = m.fuse_qr_interact = flag
            return m
    elif case == "cat":
        _, meta = load_golden("qr_training")
        c = meta["cases"]["mult"]

        def build(flag):
            np.random.seed(5)
            torch.manual_seed(5)
            m = dlrm_amd.DLRM_Net(c["m_spa"], np.asarray(c["ln_emb"]), np.asarray(c["ln_bot"]),
                                  np.asarray([c["m_spa"] * (1 + len(c["ln_emb"])), 32, 1]), "cat", sigmoid_top=1, loss_function="bce",
                                  qr_flag=True, qr_operation="mult", qr_collisions=4, qr_threshold=meta["qr_threshold"]).to(dev())
            m.fuse_narrow_interact = m.fuse_qr_interact = flag
            return m
    else:
        def build(flag):
            return qr_model(cfg, flag, flag)
    on, off = build(True), build(False)
    assert on._has_qr(on.emb_l) == (case != "md")
    X, lS_o, lS_i, _ = batch(cfg, 41, B, hots=hots)          # (the MD fixture has the same five row counts)
    want = predict(off, X, lS_o, lS_i)
    calls = counted(monkeypatch)
    got = predict(on, X, lS_o, lS_i)
    assert calls.n["interact_fwd_gather_narrow_qr"] == 0 and calls.n["interact_fwd_gather_qr"] == 0
    assert calls.n["emb_fwd_qr"] == (0 if case == "md" else 1)
    assert same_bits(got, want)
    ops.check_index_errors(sync=True)


def test_offsets_state_of_a_capturing_step_gives_the_two_kernel_form(monkeypatch):
    """While a HIP graph is being captured ops.offsets_iota_state answers None (undecided), and the narrow branches then keep the two-kernel
    form.  GraphedTrainStep itself refuses QR tables (tests/test_gpu_qr_emb.py), so the answer of a capturing step is put in place of the
    function: the flags-on model must run the flags-off model's kernels and give its bits."""
    from dlrm_amd import ops
    cfg = "d16_mult"
    on, off = qr_model(cfg, True, True, ops.UPD_DETERMINISTIC), qr_model(cfg, False, False, ops.UPD_DETERMINISTIC)
    X, lS_o, lS_i, target = batch(cfg, 70, state="fresh")
    want = predict(off, X, lS_o, lS_i)
    l_off = one_step(off, torch.optim.SGD(off.parameters(), lr=0.1), X, lS_o, lS_i, target)
    asked = []
    monkeypatch.setattr(ops, "offsets_iota_state", lambda o: asked.append(1))          # (returns None)
    calls = counted(monkeypatch)
    assert same_bits(predict(on, X, lS_o, lS_i), want)
    assert asked and calls.counts() == (0, 0, 1, 0, 1, 0, 0, 0)
    assert one_step(on, torch.optim.SGD(on.parameters(), lr=0.1), X, lS_o, lS_i, target) == l_off
    assert calls.counts() == (0, 0, 2, 1, 2, 1, 0, 0)
    same_parameters(on, off)


def test_update_in_backward_keeps_the_step_time_update(monkeypatch):
    from dlrm_amd import ops
    cfg = "d16_mult"
    on, off = qr_model(cfg, True, True, ops.UPD_DETERMINISTIC), qr_model(cfg, False, False, ops.UPD_DETERMINISTIC)
    on.update_in_backward = True
    presorts = []
    p0 = ops.emb_presort
    monkeypatch.setattr(ops, "emb_presort", lambda *a, **k: presorts.append(1) or p0(*a, **k))
    calls = counted(monkeypatch)
    o_on, o_off = torch.optim.SGD(on.parameters(), lr=0.1), torch.optim.SGD(off.parameters(), lr=0.1)
    for s in range(2):                                 # (the optimizer is bound at the first step: the second backward could update)
        X, lS_o, lS_i, target = batch(cfg, 30 + s)
        assert one_step(on, o_on, X, lS_o, lS_i, target) == one_step(off, o_off, X, lS_o, lS_i, target)
    assert not presorts
    assert calls.counts() == (2, 2, 2, 2, 2, 2, 0, 0)              # two fused steps of `on`, two two-kernel steps of `off`
    same_parameters(on, off)


def test_evaluate_inference_takes_the_fused_forward(monkeypatch):
    from dlrm_amd import evaluate
    cfg = "d64_mult"
    on, off = qr_model(cfg, True, True), qr_model(cfg, False, False)
    batches = []
    for s in range(2):
        X, lS_o, lS_i, Tg = batch(cfg, 50 + s, state="fresh")
        batches.append((X.cpu(), [o.cpu() for o in lS_o], [i.cpu() for i in lS_i], Tg.cpu()))
    want = evaluate.inference(off, batches, device=dev())
    calls = counted(monkeypatch)
    got = evaluate.inference(on, batches, device=dev())
    assert calls.n["interact_fwd_gather_narrow_qr"] == 2 and calls.n["interact_bwd_gather_narrow_qr"] == 0
    assert got == want


@pytest.mark.parametrize("tagged", [True, False])
@pytest.mark.parametrize("cfg", ["d16_mult", "d64_add"])
def test_backward_twice_through_a_retained_graph(cfg, tagged):
    """nothing the backward needs is consumed by it (the rows are fetched again; on the device-flag path the sums stay with the node)"""
    from dlrm_amd import ops
    model = qr_model(cfg, True, True)
    D = 16 if cfg.startswith("d16") else 64
    X, lS_o, lS_i, T = batch(cfg, 60, state="tagged" if tagged else "fresh")
    E = model.loss_fn(model(X, lS_o, lS_i), T)
    E.backward(retain_graph=True)
    E.backward()
    assert len(model._pending_emb) == 2
    (w1, _, g1, _), (_, _, g2, _) = model._pending_emb
    Tv = len(list(model._emb_weights(model.emb_l)))
    assert len(w1) == Tv and g1.size(1) == Tv * D            # the virtual table list
    assert torch.equal(g1, g2)
    model._pending_emb.clear()
    ops.check_index_errors(sync=True)
