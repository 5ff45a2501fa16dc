"""The DCN-v2 elementwise halves, the fused cross GEMM epilogue, the addend epilogue, the loss / clamp kernels and the pooling-weight kernels
(csrc/loss_opt.hip, csrc/gemm.hip + gemm_bf16.hip, csrc/emb.hip) through dlrm_amd.ops, against the float64 references of
tests/test_elementwise_host.py (each proven there against torch's CPU operators) on seeded numpy inputs.

Shapes are the smallest at which each kernel can still go wrong: one element, a tail that is no multiple of 4, one block of 256 items and its
two neighbours, a grid-stride loop that wraps its capped grid, a ragged M / N tile, D beyond one wavefront, more tables than one launch takes.
Every tolerance is stated, with its reason, in the test that uses it."""
import numpy as np
import pytest
import torch

import test_elementwise_host as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ACT_NONE = 0
U24 = 2.0 ** -24                       # half an fp32 ulp, relative: the bound of ONE correctly rounded fp32 operation
TINY = 2.0 ** -126                     # smallest normal fp32: results below it may be flushed to zero


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def at_offset(a, k):
    """`a` (1-D numpy, fp32 or bf16 bit patterns as uint16) on the device as a contiguous view that starts k ELEMENTS past an allocation's
    (at least 256-byte aligned) start: k = 1 puts an fp32 operand 4 bytes, a bf16 operand 2 bytes off a 16-byte boundary"""
    if a.dtype == np.uint16:
        buf = torch.zeros(a.size + 8, dtype=torch.bfloat16, device=dev())
        buf[k:k + a.size].copy_(torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16))
    else:
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev())
        buf[k:k + a.size].copy_(torch.from_numpy(a))
    v = buf[k:k + a.size]
    assert v.data_ptr() % 16 == (k * a.itemsize) % 16
    return v


def bits16(t):
    """bf16 tensor -> its uint16 bit patterns"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_one_rounding(got, ref, what):
    """|got - ref| <= 2^-24 * |ref| + 2^-126: got is the fp32 rounding of the exact (float64) ref — half an ulp, plus the floor for flushed
    subnormals.  Two roundings (a product rounded before the sum), a wrong operand or a wrong element all exceed it."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    err = np.abs(got - ref)
    bound = U24 * np.abs(ref) + TINY
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, "%s: %d of %d beyond one rounding, first at %d: got %r want %r" % (what, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


def mixed(rng, n):
    """fp32 values over six decades, both signs"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)


# ------------------------------------------------------------------------------------------ cross halves and add
CROSS_N = [1, 3, 4, 5, 1020, 1023, 1024, 1025, 1028, 4 * 256 * 3 + 4]     # 1020 / 1024 / 1028 straddle one block of 256 float4 items


@pytest.mark.parametrize("n", CROSS_N)
def test_cross_fwd_is_one_fma_and_its_bf16_rounding(n):
    """ops.cross_fwd: out = fma(x0, u, xl), ONE rounding of the exact x0 * u + xl (a product of two fp32 values is exact in float64): bound
    2^-24 |ref| + 2^-126.  On a quarter of the elements xl = -fl(x0 * u): the fma returns the product's rounding error, separate multiply and
    add return 0.  out16 is bit-equal to the RNE rounding of the fp32 value the same call stored.  Every n runs 16-byte aligned (float4 kernel
    where n % 4 == 0, scalar kernel otherwise) and one element past a 16-byte boundary (scalar kernel): the same bits."""
    from dlrm_amd import ops
    rng = np.random.default_rng(n)
    x0, u, xl = mixed(rng, n), mixed(rng, n), mixed(rng, n)
    cancel = rng.random(n) < 0.25
    cancel[0] = True                                     # at n = 1 too
    xl[cancel] = -(x0[cancel] * u[cancel])
    ref = x0.astype(np.float64) * u.astype(np.float64) + xl.astype(np.float64)
    outs = []
    for k in (0, 1):
        a, b, c = at_offset(x0, k), at_offset(u, k), at_offset(xl, k)
        for want16 in (False, True):
            r = ops.cross_fwd(a, b, c, want16=want16)
            out = (r[0] if want16 else r).cpu().numpy()
            assert_one_rounding(out, ref, "cross_fwd n=%d offset=%d" % (n, k))
            if want16:
                assert np.array_equal(bits16(r[1]), H.round_nearest(out)), (n, k)
            outs.append(out)
    for o in outs[1:]:
        assert np.array_equal(bits32(o), bits32(outs[0]))
    assert n < 1020 or np.any((ref != 0) & cancel)       # the cancelling elements do tell an fma from two roundings


@pytest.mark.parametrize("n", CROSS_N)
@pytest.mark.parametrize("accumulate", [False, True])
def test_cross_bwd_products_accumulation_and_bf16_forms(n, accumulate):
    """ops.cross_bwd: du = g * x0 (one rounding), dx0 = fma(g, u, accumulate ? dx0_in : 0) (one rounding; dx0_in = -fl(g * u) on a quarter of
    the elements, so that the fma cancels).  accumulate False runs over a dx0 pre-filled with NaN: it must be overwritten, not read.
    out="bf16": du16 is bit-equal to the RNE rounding of the fp32 du of the out="f32" call.  u as bfloat16 (the U16 template) must give, bit
    for bit, the dx0 of the fp32 form fed the widened bf16 values: that pins which half of a packed pair is the even element.  Aligned and
    one element past a 16-byte boundary (bf16 u: 2 bytes past): the same bits."""
    from dlrm_amd import ops
    rng = np.random.default_rng(1000 + n)
    g, x0 = mixed(rng, n), mixed(rng, n)
    u16 = H.round_nearest(mixed(rng, n))                 # bf16 bit patterns; distinct neighbours, so swapped halves cannot go unnoticed
    u = H.bf16_to_f32(u16)
    dx0_in = mixed(rng, n)
    cancel = rng.random(n) < 0.25
    cancel[0] = True
    dx0_in[cancel] = -(g[cancel] * u[cancel])
    du_ref = g.astype(np.float64) * x0.astype(np.float64)
    dx_ref = g.astype(np.float64) * u.astype(np.float64) + (dx0_in.astype(np.float64) if accumulate else 0.0)
    seen = []
    for k in (0, 1):
        tg, tx0, tu, tu16 = at_offset(g, k), at_offset(x0, k), at_offset(u, k), at_offset(u16, k)

        def fresh_dx0():
            return at_offset(dx0_in if accumulate else np.full(n, np.nan, dtype=np.float32), k)

        d1 = fresh_dx0()
        du = ops.cross_bwd(tg, tx0, tu, d1, accumulate, out="f32")
        d2 = fresh_dx0()
        du16 = ops.cross_bwd(tg, tx0, tu, d2, accumulate, out="bf16")
        d3 = fresh_dx0()
        du_b = ops.cross_bwd(tg, tx0, tu16, d3, accumulate, out="f32")
        d4 = fresh_dx0()
        du16_b = ops.cross_bwd(tg, tx0, tu16, d4, accumulate, out="bf16")
        du_np, d1_np = du.cpu().numpy(), d1.cpu().numpy()
        what = "cross_bwd n=%d offset=%d accumulate=%d" % (n, k, accumulate)
        assert_one_rounding(du_np, du_ref, what + " du")
        assert_one_rounding(d1_np, dx_ref, what + " dx0")
        assert du16.dtype == torch.bfloat16 and np.array_equal(bits16(du16), H.round_nearest(du_np)), what
        assert np.array_equal(bits16(du16_b), H.round_nearest(du_np)), what
        assert np.array_equal(bits32(du_b.cpu().numpy()), bits32(du_np)), what
        for d in (d2, d3, d4):
            assert np.array_equal(bits32(d.cpu().numpy()), bits32(d1_np)), what
        seen.append((du_np, d1_np))
    assert np.array_equal(bits32(seen[0][0]), bits32(seen[1][0])) and np.array_equal(bits32(seen[0][1]), bits32(seen[1][1]))


@pytest.mark.parametrize("n", CROSS_N)
def test_add_is_one_rounded_sum(n):
    """ops.add: out = a + b, one rounding of the float64 sum (2^-24 |ref| + 2^-126); b = -a(1 + 2^-20) on a quarter of the elements."""
    from dlrm_amd import ops
    rng = np.random.default_rng(2000 + n)
    a, b = mixed(rng, n), mixed(rng, n)
    cancel = rng.random(n) < 0.25
    b[cancel] = -(a[cancel] * np.float32(1 + 2.0 ** -20))
    ref = a.astype(np.float64) + b.astype(np.float64)
    outs = []
    for k in (0, 1):
        out = ops.add(at_offset(a, k), at_offset(b, k)).cpu().numpy()
        assert_one_rounding(out, ref, "add n=%d offset=%d" % (n, k))
        outs.append(out)
    assert np.array_equal(bits32(outs[0]), bits32(outs[1]))


# ------------------------------------------------------------------------------------------ fused cross GEMM, addend epilogue
GEMM_SHAPES = [(256, 192, 64), (257, 196, 64), (300, 452, 192), (777, 260, 128)]     # one tile at the lower limits; ragged M and N tiles


def _bf16_operands(rng, M, N, K):
    A = to_dev(rng.standard_normal((M, K)).astype(np.float32)).to(torch.bfloat16)
    B = to_dev((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).to(torch.bfloat16)
    return A, B


def _padded(a, pad=4, fill=float("nan")):
    """[M, N] numpy -> a [:, :N] device view of an [M, N + pad] buffer whose padding columns hold `fill` (row stride N + pad)"""
    M, N = a.shape
    buf = torch.full((M, N + pad), fill, dtype=torch.float32, device=dev())
    buf[:, :N].copy_(torch.from_numpy(a))
    return buf, buf[:, :N]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("want16", [True, False], ids=["out16", "f32only"])
def test_gemm_bf16_cross_equals_product_then_cross_fwd(M, N, K, with_bias, want16):
    """ops.gemm_bf16_cross (the `mul` / `Ub` epilogue of the bf16-shaped kernel) at one tile and at ragged M / N tiles:
      * x_next BIT-identical to ops.gemm_bf16 (fp32 u) followed by ops.cross_fwd — the same fma on the same u;
      * u16 bit-equal to the RNE rounding of that u, out16 to the RNE rounding of x_next;
      * u itself against a float64 product of the same bf16 operands at rtol 2e-5, atol 3e-5 (test_gemm_bf16_phased_kernel's bar: fp32
        accumulation of K exact bf16 products).
    x0 and xl are row-padded views (stride N + 4, NaN in the padding): a kernel that ignored a leading dimension would read the NaN."""
    from dlrm_amd import ops
    rng = np.random.default_rng(M + N + K)
    v16, W16 = _bf16_operands(rng, M, N, K)
    bias = to_dev(rng.standard_normal(N).astype(np.float32)) if with_bias else None
    u = torch.full((M, N), float("nan"), device=dev())
    ops.gemm_bf16(v16, W16, bias, ACT_NONE, u, None)
    u_np = u.cpu().numpy()
    want_u = v16.double().cpu().numpy() @ W16.double().cpu().numpy().T + (bias.double().cpu().numpy() if with_bias else 0.0)
    np.testing.assert_allclose(u_np, want_u, rtol=2e-5, atol=3e-5)
    x0 = rng.standard_normal((M, N)).astype(np.float32)
    xl = rng.standard_normal((M, N)).astype(np.float32)
    cancel = rng.random((M, N)) < 0.25
    xl[cancel] = -(x0[cancel] * u_np[cancel])
    _, x0v = _padded(x0)
    _, xlv = _padded(xl)
    want = ops.cross_fwd(to_dev(x0), u, to_dev(xl))
    fused = ops.gemm_bf16_cross(v16, W16, bias, x0v, xlv, want16=want16)
    assert fused is not None, "the bf16-shaped kernel must take (%d, %d, %d)" % (M, N, K)
    out, out16, ub = fused
    torch.cuda.synchronize()
    assert torch.equal(out, want), float((out - want).abs().max())
    assert np.array_equal(bits16(ub), H.round_nearest(u_np).reshape(-1))
    if want16:
        assert np.array_equal(bits16(out16), H.round_nearest(out.cpu().numpy()).reshape(-1))
    else:
        assert out16 is None
    assert_one_rounding(out.cpu().numpy(), x0.astype(np.float64).reshape(-1) * u_np.astype(np.float64).reshape(-1) + xl.astype(np.float64).reshape(-1),
                        "gemm_bf16_cross x_next")


@pytest.mark.parametrize("M,N,K", [(256, 192, 32), (255, 192, 64), (256, 188, 64)], ids=["K32", "M255", "N188"])
def test_gemm_bf16_cross_declines_outside_its_preconditions(M, N, K):
    """K = 32 passes the entry point's own checks (K % 32 == 0) but not the bf16-shaped kernel's (K % 64 == 0, M >= 256, N >= 192): the call
    returns None — the caller keeps the two kernels — and raises nothing."""
    from dlrm_amd import ops
    rng = np.random.default_rng(M + N + K)
    v16, W16 = _bf16_operands(rng, M, N, K)
    x0, xl = to_dev(rng.standard_normal((M, N)).astype(np.float32)), to_dev(rng.standard_normal((M, N)).astype(np.float32))
    assert ops.gemm_bf16_cross(v16, W16, None, x0, xl, want16=True) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bf16_addends_equal_product_then_adds(M, N, K):
    """`addend` / `addend2` of ops.gemm_bf16 (the DCN-v2 backward's g + dv.V and dx0 + g + dv.V):
      * Cf against float64 A.B^T + addend (+ addend2) at rtol 2e-5, atol 3e-5 (the product's bar; the adds are exact in float64) — the atol is
        scaled by nothing: addends are N(0, 1) like the product;
      * BIT-identical to the plain product followed by ops.add once, or twice in the kernel's order (addend first);
      * in place: Cf the same tensor as addend2, and in a second case as addend — the bits of the out-of-place call.
    Cf is a row-padded view (stride N + 4) whose padding holds 7.0 and must keep it; the addends are padded views with NaN in the padding."""
    from dlrm_amd import ops
    rng = np.random.default_rng(7 * M + N + K)
    A, B = _bf16_operands(rng, M, N, K)
    a1, a2 = rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    P = torch.full((M, N), float("nan"), device=dev())
    ops.gemm_bf16(A, B, None, ACT_NONE, P, None)
    prod = A.double().cpu().numpy() @ B.double().cpu().numpy().T
    _, a1v = _padded(a1)
    _, a2v = _padded(a2)
    # one addend
    buf1, C1 = _padded(np.zeros((M, N), dtype=np.float32), fill=7.0)
    ops.gemm_bf16(A, B, None, ACT_NONE, C1, None, addend=a1v)
    np.testing.assert_allclose(C1.cpu().numpy(), prod + a1.astype(np.float64), rtol=2e-5, atol=3e-5)
    s1 = ops.add(P, to_dev(a1))
    assert torch.equal(C1, s1)
    # two addends
    buf2, C2 = _padded(np.zeros((M, N), dtype=np.float32), fill=7.0)
    ops.gemm_bf16(A, B, None, ACT_NONE, C2, None, addend=a1v, addend2=a2v)
    np.testing.assert_allclose(C2.cpu().numpy(), prod + a1.astype(np.float64) + a2.astype(np.float64), rtol=2e-5, atol=3e-5)
    assert torch.equal(C2, ops.add(s1, to_dev(a2)))
    assert bool(torch.all(buf1[:, N:] == 7.0)) and bool(torch.all(buf2[:, N:] == 7.0))
    # in place over addend2 (layer 0 of the DCN-v2 backward: dx0 = dx0 + g + dv.V), then over addend (gsum = gsum + dv.V)
    _, io = _padded(a2)
    ops.gemm_bf16(A, B, None, ACT_NONE, io, None, addend=a1v, addend2=io)
    assert torch.equal(io, C2)
    _, io = _padded(a1)
    ops.gemm_bf16(A, B, None, ACT_NONE, io, None, addend=io)
    assert torch.equal(io, C1)
    _, io = _padded(a1)
    ops.gemm_bf16(A, B, None, ACT_NONE, io, None, addend=io, addend2=a2v)
    assert torch.equal(io, C2)


def test_gemm_bf16_addend_refusals_write_nothing():
    """addend2 without addend, an addend that is not 16-byte aligned, and an addend on a shape the bf16-shaped kernel does not take (M = 128:
    the fp32-shaped kernel has no addend operand) each raise through _lib.check and leave Cf as it was."""
    from dlrm_amd import ops
    rng = np.random.default_rng(5)
    M, N, K = 256, 192, 64
    A, B = _bf16_operands(rng, M, N, K)
    ad = to_dev(rng.standard_normal((M, N)).astype(np.float32))
    flat = torch.zeros(M * N + 4, device=dev())
    off1 = flat[1:1 + M * N].view(M, N)                                 # 4 bytes past a 16-byte boundary
    C = torch.full((M, N), 7.0, device=dev())
    with pytest.raises(RuntimeError, match="dlrm_gemm_bf16"):
        ops.gemm_bf16(A, B, None, ACT_NONE, C, None, addend2=ad)
    with pytest.raises(RuntimeError, match="DLRM_E_ALIGN"):
        ops.gemm_bf16(A, B, None, ACT_NONE, C, None, addend=off1)
    with pytest.raises(RuntimeError, match="DLRM_E_ALIGN"):
        ops.gemm_bf16(A, B, None, ACT_NONE, C, None, addend=ad, addend2=off1)
    A2 = A[:128]
    C128 = torch.full((128, N), 7.0, device=dev())
    with pytest.raises(RuntimeError, match="DLRM_E_MODE"):
        ops.gemm_bf16(A2, B, None, ACT_NONE, C128, None, addend=ad[:128])
    torch.cuda.synchronize()
    assert bool(torch.all(C == 7.0)) and bool(torch.all(C128 == 7.0))
    ops.gemm_bf16(A2, B, None, ACT_NONE, C128, None)                     # the same shape without an addend runs (fp32-shaped kernel)
    torch.cuda.synchronize()
    np.testing.assert_allclose(C128.cpu().numpy(), A2.double().cpu().numpy() @ B.double().cpu().numpy().T, rtol=2e-5, atol=3e-5)


# ------------------------------------------------------------------------------------------ losses
LOSS_B = [1, 3, 1023, 1024, 1025, 4097]            # one block covers 1024 samples; 4097 gives five partials


def _targets(rng, B):
    """0 / 1 targets with a quarter fractional; 0.3, 0.999, 1.0, 0.0 at fixed places when there is room"""
    t = np.round(rng.random(B)).astype(np.float32)
    frac = rng.random(B) < 0.25
    t[frac] = rng.random(int(frac.sum())).astype(np.float32)
    if B >= 8:
        t[4:8] = [0.3, 0.999, 1.0, 0.0]
    return t


def _spread(B, values, rng, base):
    """`base` with `values` written at distinct random places (as many as fit)"""
    k = min(B, len(values))
    pos = rng.permutation(B)[:k]
    base[pos] = np.asarray(values, dtype=np.float32)[rng.permutation(len(values))[:k]]
    return base, pos


@pytest.mark.parametrize("B", LOSS_B)
@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_bce_logits_loss_and_gradient(B, grad_scale):
    """ops.bce_logits_loss: targets 0 / 1 and fractional, logits N(0, 3) plus 0, +-1e-8, +-30, +-88.5, +-104, +-1e4 (each with every kind of
    target when B allows: the extremes are written three times).
    Loss: relative 1e-5, the bar test_bce_and_mse sets for these block reductions.
    Gradient: |got - ref| <= 1e-5 |ref| + 4 * 2^-24 * grad_scale / B.  The absolute term: sigmoid(x) next to 1 carries an fp32 rounding error
    of a few 2^-24 that the exact subtraction of t = 1 turns into an absolute error of the difference.
    Nothing may be NaN or inf, at +-1e4 either (expf overflows beyond 88.7).  want_grad False returns None and the same loss bits."""
    from dlrm_amd import ops
    rng = np.random.default_rng(B)
    x = (rng.standard_normal(B) * 3).astype(np.float32)
    x, pos = _spread(B, np.repeat(H.LOGIT_EXTREMES, 3), rng, x)
    t = _targets(rng, B)
    t[pos] = np.resize(np.array([0.0, 1.0, 0.25], dtype=np.float32), pos.size)
    want, gwant = H.bce_logits_ref(x, t, grad_scale)
    loss, dz = ops.bce_logits_loss(to_dev(x), to_dev(t), grad_scale, True)
    loss2, none = ops.bce_logits_loss(to_dev(x), to_dev(t), grad_scale, False)
    torch.cuda.synchronize()
    got, g = float(loss.cpu()), dz.cpu().numpy().astype(np.float64)
    assert none is None and torch.equal(loss, loss2)
    assert np.isfinite(got) and np.all(np.isfinite(g))
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    err, bound = np.abs(g - gwant), 1e-5 * np.abs(gwant) + 4 * U24 * grad_scale / B
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (bad[:4], x[bad[:4]], t[bad[:4]], g[bad[:4]], gwant[bad[:4]])


@pytest.mark.parametrize("B", LOSS_B)
@pytest.mark.parametrize("use_weights", [False, True], ids=["noweights", "weights"])
@pytest.mark.parametrize("class_weights,grad_scale", [((1.0, 1.0), 1.0), ((0.3, 2.5), 0.37), ((0.3, 2.5), 1.0)])
def test_weighted_bce_loss_and_gradient(B, use_weights, class_weights, grad_scale):
    """ops.bce_loss with per-sample weights, class weights (w_neg, w_pos), fractional targets among the 0 / 1 ones and a gradient scale; p
    holds 0, 1, 1e-30 and 1 - 2^-24 (log clamp at -100, denominator floor 1e-12).  Tolerances of test_bce_and_mse: loss relative 1e-5,
    gradient rtol 1e-5 / atol 1e-12.  want_grad False: None and the same loss bits."""
    from dlrm_amd import ops
    rng = np.random.default_rng(10 * B + int(use_weights))
    p = rng.random(B).astype(np.float32)
    p, pos = _spread(B, np.repeat(H.P_EXTREMES, 4), rng, p)
    t = _targets(rng, B)
    t[pos] = np.resize(np.array([0.0, 1.0, 0.3, 0.999], dtype=np.float32), pos.size)
    w = (rng.random(B) + 0.5).astype(np.float32) if use_weights else None
    want, gwant = H.bce_ref(p, t, w, class_weights, grad_scale)
    wd = to_dev(w) if use_weights else None
    loss, dp = ops.bce_loss(to_dev(p), to_dev(t), wd, grad_scale, True, class_weights=class_weights)
    loss2, none = ops.bce_loss(to_dev(p), to_dev(t), wd, grad_scale, False, class_weights=class_weights)
    torch.cuda.synchronize()
    assert none is None and torch.equal(loss, loss2)
    assert abs(float(loss.cpu()) - want) <= 1e-5 * max(abs(want), 1e-6), (float(loss.cpu()), want)
    np.testing.assert_allclose(dp.cpu().numpy(), gwant, rtol=1e-5, atol=1e-12)


def test_weighted_bce_fractional_target_takes_w_neg():
    """Two calls that differ in the class weights only: the gradient of a sample with t = 0.999 (and of one with t = 0.3, and t = 0) moves by
    w_neg = 0.3, that of a sample with t = 1 by w_pos = 2.5 — `loss_ws[T.long()]` truncates.  One rounding of the weight product: 1e-6."""
    from dlrm_amd import ops
    p = np.array([0.2, 0.6, 0.7, 0.9, 0.4], dtype=np.float32)
    t = np.array([0.999, 1.0, 0.3, 0.0, 1.0], dtype=np.float32)
    _, d1 = ops.bce_loss(to_dev(p), to_dev(t), None, 1.0, True, class_weights=(1.0, 1.0))
    l2, d2 = ops.bce_loss(to_dev(p), to_dev(t), None, 1.0, True, class_weights=(0.3, 2.5))
    ratio = (d2 / d1).cpu().numpy()
    np.testing.assert_allclose(ratio, [0.3, 2.5, 0.3, 0.3, 2.5], rtol=1e-6)
    want, _ = H.bce_ref(p, t, None, (0.3, 2.5))
    assert abs(float(l2.cpu()) - want) <= 1e-5 * want


EW_N = [1, 255, 257, 2048 * 256 + 3]               # the last wraps the grid-stride loop: the grid is capped at 2048 blocks of 256


@pytest.mark.parametrize("n", EW_N)
def test_bce_elementwise_and_backward(n):
    """ops.bce_elementwise / _bwd (BCELoss(reduction="none")): per element rtol 1e-5 (a handful of fp32 roundings and two libm calls of same-signed
    terms; no absolute term is needed: nothing cancels); the clamp cases exact: p = 0, t = 1 and p = 1, t = 0 give exactly 100."""
    from dlrm_amd import ops
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(np.float32)
    p, pos = _spread(n, np.repeat(H.P_EXTREMES, 4), rng, p)
    t = _targets(rng, n)
    t[pos] = np.resize(np.array([0.0, 1.0, 0.3, 0.999], dtype=np.float32), pos.size)
    if n >= 255:
        p[-1], t[-1], p[-2], t[-2] = 0.0, 1.0, 1.0, 0.0            # the clamp cases, in the tail / in the wrapped part of the loop
    dloss = rng.standard_normal(n).astype(np.float32)
    pd, td = to_dev(p), to_dev(t)
    loss = ops.bce_elementwise(pd, td).cpu().numpy()
    dp = ops.bce_elementwise_bwd(pd, td, to_dev(dloss)).cpu().numpy()
    np.testing.assert_allclose(loss, H.bce_elementwise_ref(p, t), rtol=1e-5, atol=0)
    np.testing.assert_allclose(dp, H.bce_elementwise_bwd_ref(p, t, dloss), rtol=1e-5, atol=0)
    if n >= 255:
        assert loss[-1] == 100.0 and loss[-2] == 100.0


@pytest.mark.parametrize("n", [1, 257, 1024 * 256 + 5])          # the grid is capped at 1024 blocks
def test_scale_by_device_scalar_is_the_fp32_product(n):
    from dlrm_amd import ops
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    s = np.float32(0.37)
    y = ops.scale_by_scalar(to_dev(x), to_dev(np.array([s], dtype=np.float32))).cpu().numpy()
    assert np.array_equal(bits32(y), bits32(x * s))


@pytest.mark.parametrize("lo,hi", [(0.01, 0.99), (-1.5, 2.25), (0.5, 0.5)])
@pytest.mark.parametrize("n", [11, 2048 * 256 + 3])
def test_clamp_and_backward_are_torch_clamp_and_the_inclusive_mask(lo, hi, n):
    """ops.clamp / ops.clamp_bwd: bit-equal to torch.clamp and to dy * (lo <= x <= hi).  Inputs sit exactly on lo and on hi (the gradient
    passes), one fp32 step outside each (it does not) and one inside; lo == hi; n = 2048 * 256 + 3 wraps the capped grid, with the boundary
    inputs again in its tail."""
    from dlrm_amd import ops
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    rng = np.random.default_rng(n)
    edge = H.clamp_boundary_inputs(lo, hi)
    x = rng.standard_normal(n).astype(np.float32)
    x[:edge.size] = edge
    x[-edge.size:] = edge
    dy = rng.standard_normal(n).astype(np.float32)
    xd = to_dev(x)
    y = ops.clamp(xd, lo, hi).cpu().numpy()
    dx = ops.clamp_bwd(xd, lo, hi, to_dev(dy)).cpu().numpy()
    assert np.array_equal(bits32(y), bits32(torch.clamp(torch.from_numpy(x), lo, hi).numpy()))
    assert np.array_equal(bits32(y), bits32(H.clamp_ref(x, np.float32(lo), np.float32(hi))))
    assert np.array_equal(bits32(dx), bits32(H.clamp_bwd_ref(x, np.float32(lo), np.float32(hi), dy)))
    assert dx[0] == dy[0] and dx[1] == dy[1] and dx[2] == 0 and dx[4] == 0


# ------------------------------------------------------------------------------------------ pooling weights
def _pool_case(T, D, B, max_len, np_dtype, seed):
    """T tables with DISTINCT row counts (table 0: a single row, every lookup collides on one address), ragged bags with empty ones, the last
    bag forced full / empty / left alone in turn"""
    rng = np.random.default_rng(seed)
    rows = [1] + [5 + 3 * t for t in range(1, T)]
    Ws = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    vWs = [rng.standard_normal(n).astype(np.float32) for n in rows]
    bags = [H.ragged_bags(rng, B, n, max_len, last=("full", "empty", None)[t % 3], dtype=np_dtype) for t, n in enumerate(rows)]
    dout = rng.standard_normal((B, T * D)).astype(np.float32)
    return rng, rows, Ws, vWs, bags, dout


def _check_psw_grad(got, W, idx, off, dout_t, what):
    """rows never looked up: exactly 0.  Looked-up rows: |got[r] - ref[r]| <= (D + c_r) * 2^-24 * S_r, c_r the lookups of row r and S_r the float64
    sum of |dout_d * W_rd| over all of them: the standard bound for a sum of D * c_r fp32 terms accumulated in ANY order (a chain of at most
    D + c_r roundings on any term's path: the wave-wide dot, then the atomics, whose order is free — no tighter claim holds).  A lost
    lookup, a wrong bag end or a dropped column beyond lane 63 exceeds it by orders of magnitude."""
    ref, c, S = H.psw_grad_ref(W, idx, off, dout_t)
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got)), what
    assert np.all(got[c == 0] == 0), what
    bad = np.flatnonzero(np.abs(got - ref) > (W.shape[1] + c) * U24 * S)
    assert bad.size == 0, (what, bad[:4], got[bad[:4]], ref[bad[:4]], c[bad[:4]])


@pytest.mark.parametrize("T,D,B,max_len,idx_dtype", [(3, 12, 67, 5, torch.int64), (3, 64, 300, 3, torch.int32), (2, 65, 129, 4, torch.int64),
                                                     (2, 200, 33, 6, torch.int32), (33, 16, 40, 2, torch.int64)])
def test_pool_weights_gather_and_gradient(T, D, B, max_len, idx_dtype):
    """ops.pool_weights_gather: bit-equal to vW[idx]; attached to the bags, so that a following ops.emb_fwd equals the oracle's
    emb_fwd(..., psw=...) bit for bit (the bar of test_emb_fwd_bit_exact).  ops.emb_psw_grad: see _check_psw_grad; the result is an OUTPUT
    (`like` holds NaN, and so does freed memory of the same sizes just before the call).  D = 65 and 200 go beyond one wavefront, T = 33
    beyond one launch (32 tables), B = 67 / 129 / 33 leave a partly filled last block of 4 bags, dout is a row-padded view."""
    from dlrm_amd import ops
    np_dtype = np.int64 if idx_dtype == torch.int64 else np.int32
    rng, rows, Ws, vWs, bags, dout = _pool_case(T, D, B, max_len, np_dtype, seed=T * 1000 + D)
    assert any(o[-1] == i.size for o, i in bags) and any(o[-1] < i.size for o, i in bags)          # an empty last bag and a non-empty one
    dW, dvW = [to_dev(W) for W in Ws], [to_dev(v) for v in vWs]
    bb = ops.BagBatch([to_dev(o) for o, _ in bags], [to_dev(i) for _, i in bags])
    psw = ops.pool_weights_gather(dvW, bb)
    torch.cuda.synchronize()
    for t in range(T):
        assert np.array_equal(bits32(psw[t].cpu().numpy()), bits32(H.psw_gather_ref(vWs[t], bags[t][1]))), t
    out = torch.full((B, T * D), float("nan"), device=dev())
    ops.emb_fwd(dW, bb, out)
    want = np.concatenate([O.emb_fwd(Ws[t], bags[t][1], bags[t][0], psw=H.psw_gather_ref(vWs[t], bags[t][1])) for t in range(T)], axis=1)
    assert np.array_equal(out.cpu().numpy(), want)
    buf = torch.full((B, T * D + 4), float("nan"), device=dev())
    buf[:, :T * D].copy_(torch.from_numpy(dout))
    like = [torch.full_like(v, float("nan")) for v in dvW]
    poison = [torch.full_like(v, float("nan")) for v in dvW]
    del poison                                                     # the allocator hands these blocks to the call's torch.empty_like
    got = ops.emb_psw_grad(dW, bb, buf[:, :T * D], like)
    torch.cuda.synchronize()
    ops.check_index_errors(sync=True)
    for t in range(T):
        assert got[t].shape == (rows[t],)
        _check_psw_grad(got[t].cpu().numpy(), Ws[t], bags[t][1], bags[t][0], dout[:, t * D:(t + 1) * D], "table %d" % t)


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_pool_weights_out_of_range_id_is_skipped_and_reported(idx_dtype):
    """One id == rows in one table: the gather writes 0 for it and ops.check_index_errors(sync=True) reports it (as
    test_out_of_range_index_is_skipped_and_reported shows for the lookup); the gradient call skips that lookup — its result is the gradient of
    the batch WITHOUT it, every row of every table within the bound of _check_psw_grad — and reports nothing more."""
    from dlrm_amd import ops
    np_dtype = np.int64 if idx_dtype == torch.int64 else np.int32
    T, D, B = 3, 12, 67
    rng, rows, Ws, vWs, bags, dout = _pool_case(T, D, B, 5, np_dtype, seed=99)
    off1, idx1 = bags[1]
    j = idx1.size // 2
    bad = idx1.copy()
    bad[j] = rows[1]
    dW, dvW = [to_dev(W) for W in Ws], [to_dev(v) for v in vWs]
    bb = ops.BagBatch([to_dev(o) for o, _ in bags], [to_dev(bad if t == 1 else i) for t, (_, i) in enumerate(bags)])
    ops.check_index_errors(sync=True)                              # clean slate
    psw = ops.pool_weights_gather(dvW, bb)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    want1 = H.psw_gather_ref(vWs[1], idx1)
    want1[j] = 0
    assert np.array_equal(bits32(psw[1].cpu().numpy()), bits32(want1))
    for t in (0, 2):
        assert np.array_equal(bits32(psw[t].cpu().numpy()), bits32(H.psw_gather_ref(vWs[t], bags[t][1])))
    got = ops.emb_psw_grad(dW, bb, to_dev(dout), [torch.full_like(v, float("nan")) for v in dvW])
    ops.check_index_errors(sync=True)                              # the gradient kernel skips without reporting again
    bag_j = int(H.bag_of_lookup(off1, idx1.size)[j])
    off_wo = off1.copy()
    off_wo[bag_j + 1:] -= 1
    for t in range(T):
        o, i = (off_wo, np.delete(idx1, j)) if t == 1 else bags[t]
        _check_psw_grad(got[t].cpu().numpy(), Ws[t], i, o, dout[:, t * D:(t + 1) * D], "table %d" % t)


# ------------------------------------------------------------------------------------------ the DCN-v2 model at an odd feature width
def test_dlrm_dcn_odd_width_odd_batch_matches_a_torch_composition():
    """DLRM_DCN with D = 5 and two tables (n = 15 features) at B = 67: B * n = 1005 is no multiple of 4, so every elementwise half of the cross
    network runs its scalar kernel.  One forward + backward + SGD step against the same model composed of torch CPU operators with autograd,
    at the tolerances of test_dlrm_dcn_model_trains_like_a_torch_composition (tests/test_gpu_model.py)."""
    import torch.nn.functional as Fn
    from dlrm_amd.optim import FusedSGD
    from dlrm_amd.torchrec_variant import DLRM_DCN
    rng = np.random.default_rng(13)
    D, rows, B, hot = 5, [40, 9], 67, [2, 1]
    np.random.seed(3)
    model = DLRM_DCN(rows, D, 13, [24, D], [32, 1], dcn_num_layers=2, dcn_low_rank_dim=8)
    with torch.no_grad():
        for b_ in model.crossnet.bias:
            b_.copy_(torch.from_numpy((rng.standard_normal(b_.shape) * 0.1).astype(np.float32)))
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    model = model.to(dev())
    opt = FusedSGD(model.parameters(), lr=0.2)
    ropt = torch.optim.SGD(list(ref.values()), lr=0.2)
    X = torch.from_numpy(rng.random((B, 13)).astype(np.float32))
    idx = [torch.from_numpy(rng.integers(0, n, size=B * h)) for n, h in zip(rows, hot)]
    off = [torch.arange(B) * h for h in hot]
    T = torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    logits = model(X.to(dev()), [o.to(dev()) for o in off], [i.to(dev()) for i in idx])
    E = model.loss_fn(logits, T.to(dev()))
    x = X
    for i in range(2):
        x = torch.relu(Fn.linear(x, ref[f"bot_l.{2 * i}.weight"], ref[f"bot_l.{2 * i}.bias"]))
    ly = [Fn.embedding_bag(idx[k], ref[f"emb_l.{k}.weight"], off[k], mode="sum", sparse=False) for k in range(len(rows))]
    x0 = torch.cat([x] + ly, dim=1)
    assert x0.shape == (67, 15)
    xl = x0
    for l in range(2):
        xl = x0 * (Fn.linear(Fn.linear(xl, ref[f"crossnet.V_kernels.{l}"]), ref[f"crossnet.W_kernels.{l}"]) + ref[f"crossnet.bias.{l}"]) + xl
    z = torch.relu(Fn.linear(xl, ref["top_l.0.weight"], ref["top_l.0.bias"]))
    rl = Fn.linear(z, ref["top_l.2.weight"], ref["top_l.2.bias"])
    RE = Fn.binary_cross_entropy_with_logits(rl, T)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), rl.detach().numpy(), rtol=5e-5, atol=5e-6)
    assert abs(float(E.detach()) - float(RE.detach())) <= 1e-5 * abs(float(RE.detach()))
    opt.zero_grad(); E.backward(); opt.step()
    ropt.zero_grad(); RE.backward(); ropt.step()
    sd = model.state_dict()
    for k, v in ref.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=2e-4, atol=1e-5, err_msg=k)
