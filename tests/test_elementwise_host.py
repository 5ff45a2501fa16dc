"""Float64 numpy references of the elementwise, loss, clamp and pooling-weight kernels (csrc/loss_opt.hip, csrc/emb.hip), the part that needs no GPU.

tests/test_gpu_elementwise.py imports them as its oracle; this file proves each one against torch's CPU operators in float64 (with autograd for the
gradients), so that the GPU tests compare the kernels with something already checked:

  * BCE with logits (mean + gradient) in the kernel's stated form, against F.binary_cross_entropy_with_logits;
  * weighted BCE on probabilities: per-sample weights times the class weight `loss_ws[T.long()]` of the reference's wbce path (a fractional target
    truncates to class 0), log terms clamped at -100, gradient denominator max((1-p)*p, 1e-12), against F.binary_cross_entropy(weight=...);
  * per-sample BCE (reduction="none") and its backward;
  * clamp and its backward (inclusive mask at both bounds: torch's clamp_backward);
  * learned pooling weights: the gather psw = vW[idx] and the dense gradient dvW, against F.embedding_bag(per_sample_weights=vW[idx]);
  * RNE bfloat16 rounding / widening: the restatement of tests/test_bf16_emb_host.py, pinned here at ties and at the last finite value.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
from test_bf16_emb_host import bf16_to_f32, round_nearest  # noqa: E402,F401  (re-exported: the GPU file rounds with these)

LOGIT_EXTREMES = np.array([0.0, 1e-8, -1e-8, 30.0, -30.0, 88.5, -88.5, 104.0, -104.0, 1e4, -1e4], dtype=np.float32)
P_EXTREMES = np.array([0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24], dtype=np.float32)


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


# ------------------------------------------------------------------------------------------------ references
def bce_logits_ref(x, t, grad_scale=1.0):
    """BCEWithLogitsLoss(mean): loss = mean((1-t)*x + m + log(exp(-m) + exp(-x-m))), m = max(-x, 0); grad = (sigmoid(x) - t) * grad_scale / B.
    Returns (loss, grad [B]) in float64; finite for every finite x (exp(-m) and exp(-x-m) are both <= 1)."""
    x, t = _f64(x), _f64(t)
    m = np.maximum(-x, 0.0)
    per = (1.0 - t) * x + m + np.log(np.exp(-m) + np.exp(-x - m))
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-x))
    return float(per.mean()), (sig - t) * (float(grad_scale) / x.size)


def class_weight_ref(t, class_weights):
    """loss_ws[T.long()] with loss_ws = (w_neg, w_pos): truncation, so only t >= 1 selects w_pos (targets lie in [0, 1])"""
    t = _f64(t)
    return np.where(t >= 1.0, float(class_weights[1]), float(class_weights[0]))


def bce_elementwise_ref(p, t):
    """BCELoss(reduction="none"): -(t*max(log p, -100) + (1-t)*max(log(1-p), -100))"""
    p, t = _f64(p), _f64(t)
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p), -100.0)
        l1p = np.maximum(np.log1p(-p), -100.0)
    return -(t * lp + (1.0 - t) * l1p)


def bce_elementwise_bwd_ref(p, t, dloss):
    """dp = dloss * (p - t) / max((1-p)*p, 1e-12f): the floor is the FLOAT constant 1e-12f (9.99999996e-13), in torch's binary_cross_entropy_backward
    (for every dtype) as in the kernel"""
    p, t, dloss = _f64(p), _f64(t), _f64(dloss)
    return dloss * (p - t) / np.maximum((1.0 - p) * p, float(np.float32(1e-12)))


def bce_ref(p, t, weights=None, class_weights=(1.0, 1.0), grad_scale=1.0):
    """weighted BCELoss(mean): w_i = weights_i * class weight; returns (loss, grad [B]) in float64"""
    p, t = _f64(p), _f64(t)
    w = class_weight_ref(t, class_weights) * (1.0 if weights is None else _f64(weights))
    loss = float((w * bce_elementwise_ref(p, t)).mean())
    return loss, bce_elementwise_bwd_ref(p, t, w) * (float(grad_scale) / p.size)


def clamp_ref(x, lo, hi):
    return np.minimum(np.maximum(np.asarray(x), lo), hi)


def clamp_bwd_ref(x, lo, hi, dy):
    """gradient passes where lo <= x <= hi, both bounds included"""
    x = np.asarray(x)
    return np.where((x >= lo) & (x <= hi), np.asarray(dy), np.zeros_like(np.asarray(dy)))


def clamp_boundary_inputs(lo, hi):
    """fp32 values exactly on lo and hi, one fp32 step outside and inside each, and a few ordinary ones"""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    inf = np.float32(np.inf)
    return np.array([lo32, hi32, np.nextafter(lo32, -inf), np.nextafter(lo32, inf), np.nextafter(hi32, inf), np.nextafter(hi32, -inf),
                     lo32 - np.float32(1), hi32 + np.float32(1), np.float32(0.5) * (lo32 + hi32), np.float32(0), np.float32(-0.0)], dtype=np.float32)


def bag_of_lookup(off, nnz):
    """bag number of every lookup: bag b holds lookups off[b] .. off[b+1], the LAST one off[B-1] .. nnz"""
    off = np.asarray(off, dtype=np.int64)
    ends = np.append(off[1:], np.int64(nnz))
    return np.repeat(np.arange(off.size, dtype=np.int64), ends - off)


def psw_gather_ref(vW, idx):
    return np.asarray(vW)[np.asarray(idx, dtype=np.int64)]


def psw_grad_ref(W, idx, off, dout_t):
    """dvW[r] = sum over lookups i of row r of <dout_t[bag(i)], W[r]>  (dout_t: the [B, D] column block of this table), in float64.
    Returns (dvW [rows], c [rows] lookups per row, S [rows] sum of |dout_d * W_rd| over them: the terms of the error bound)."""
    W, dout_t = np.asarray(W, dtype=np.float64), np.asarray(dout_t, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    prod = dout_t[bag_of_lookup(off, idx.size)] * W[idx]
    dvW, S, c = np.zeros(W.shape[0]), np.zeros(W.shape[0]), np.zeros(W.shape[0], dtype=np.int64)
    np.add.at(dvW, idx, prod.sum(axis=1))
    np.add.at(S, idx, np.abs(prod).sum(axis=1))
    np.add.at(c, idx, 1)
    return dvW, c, S


def ragged_bags(rng, B, rows, max_len, empty_frac=0.2, last=None, dtype=np.int64):
    """(offsets [B], indices [nnz]) with empty bags; last="empty" / "full" forces the last bag (the one that ends at nnz, not at off[b+1])"""
    lens = rng.integers(0, max_len + 1, size=B)
    lens[rng.random(B) < empty_frac] = 0
    if last == "empty":
        lens[-1] = 0
    elif last == "full":
        lens[-1] = max_len
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(dtype)
    return off, rng.integers(0, rows, size=int(lens.sum())).astype(dtype)


# ------------------------------------------------------------------------------------------------ the references against torch
def _targets(rng, B):
    t = np.round(rng.random(B)).astype(np.float32)
    frac = rng.random(B) < 0.25
    t[frac] = rng.random(int(frac.sum())).astype(np.float32)
    if B >= 4:
        t[:4] = [0.3, 0.999, 1.0, 0.0]
    return t


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_bce_logits_reference_equals_torch(grad_scale):
    rng = np.random.default_rng(1)
    x = np.concatenate([np.repeat(LOGIT_EXTREMES, 3), (rng.standard_normal(200) * 3).astype(np.float32)])
    t = _targets(rng, x.size)
    t[:3 * LOGIT_EXTREMES.size] = np.tile(np.array([0.0, 1.0, 0.25], dtype=np.float32), LOGIT_EXTREMES.size)
    loss, grad = bce_logits_ref(x, t, grad_scale)
    tx = torch.from_numpy(x).double().requires_grad_(True)
    tl = Fn.binary_cross_entropy_with_logits(tx, torch.from_numpy(t).double())
    (tl * grad_scale).backward()
    assert np.isfinite(loss) and np.all(np.isfinite(grad))
    assert abs(loss - float(tl.detach())) <= 1e-13 * abs(float(tl.detach()))
    np.testing.assert_allclose(grad, tx.grad.numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("use_weights", [False, True])
@pytest.mark.parametrize("class_weights", [(1.0, 1.0), (0.3, 2.5)])
def test_weighted_bce_reference_equals_torch(use_weights, class_weights):
    rng = np.random.default_rng(2)
    p = np.concatenate([np.repeat(P_EXTREMES, 4), rng.random(150).astype(np.float32)])
    t = _targets(rng, p.size)
    t[:4 * P_EXTREMES.size] = np.tile(np.array([0.0, 1.0, 0.3, 0.999], dtype=np.float32), P_EXTREMES.size)
    w = (rng.random(p.size) + 0.5).astype(np.float32) if use_weights else None
    loss, grad = bce_ref(p, t, w, class_weights, 0.37)
    tp = torch.from_numpy(p).double().requires_grad_(True)
    tt = torch.from_numpy(t).double()
    loss_ws = torch.tensor(class_weights, dtype=torch.float64)
    wt = loss_ws[tt.long().view(-1)]                                   # the reference's class weights (dlrm_s_pytorch.py:388-391)
    if w is not None:
        wt = wt * torch.from_numpy(w).double()
    tl = Fn.binary_cross_entropy(tp, tt, weight=wt)
    (tl * 0.37).backward()
    assert abs(loss - float(tl.detach())) <= 1e-13 * abs(float(tl.detach()))
    np.testing.assert_allclose(grad, tp.grad.numpy(), rtol=1e-12, atol=0)
    # the truncation: 0.3 and 0.999 carry w_neg, only 1.0 carries w_pos
    assert list(class_weight_ref(np.array([0.0, 0.3, 0.999, 1.0]), (0.3, 2.5))) == [0.3, 0.3, 0.3, 2.5]


def test_per_sample_bce_reference_equals_torch():
    rng = np.random.default_rng(3)
    p = np.concatenate([np.repeat(P_EXTREMES, 4), rng.random(100).astype(np.float32)])
    t = _targets(rng, p.size)
    t[:4 * P_EXTREMES.size] = np.tile(np.array([0.0, 1.0, 0.3, 0.999], dtype=np.float32), P_EXTREMES.size)
    dloss = rng.standard_normal(p.size).astype(np.float32)
    tp = torch.from_numpy(p).double().requires_grad_(True)
    tl = Fn.binary_cross_entropy(tp, torch.from_numpy(t).double(), reduction="none")
    tl.backward(torch.from_numpy(dloss).double())
    np.testing.assert_allclose(bce_elementwise_ref(p, t), tl.detach().numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(bce_elementwise_bwd_ref(p, t, dloss), tp.grad.numpy(), rtol=1e-12, atol=0)
    assert bce_elementwise_ref(np.float32(0), np.float32(1))[0] == 100.0 and bce_elementwise_ref(np.float32(1), np.float32(0))[0] == 100.0


@pytest.mark.parametrize("lo,hi", [(0.01, 0.99), (-1.5, 2.25), (0.5, 0.5), (1e-7, 1.0 - 1e-7)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_clamp_reference_equals_torch(lo, hi, dtype):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))              # the bounds the kernel receives: fp32 values
    rng = np.random.default_rng(4)
    x = np.concatenate([clamp_boundary_inputs(lo, hi), rng.standard_normal(50).astype(np.float32)])
    dy = rng.standard_normal(x.size).astype(np.float32)
    tx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    ty = torch.clamp(tx, lo, hi)
    ty.backward(torch.from_numpy(dy).to(dtype))
    assert np.array_equal(clamp_ref(x, np.float32(lo), np.float32(hi)).astype(np.float64), ty.detach().double().numpy())
    got = clamp_bwd_ref(x, np.float32(lo), np.float32(hi), dy)
    assert np.array_equal(got.astype(np.float64), tx.grad.double().numpy())
    assert got[0] == dy[0] and got[1] == dy[1]                         # exactly on a bound: the gradient passes
    if lo < hi:
        assert got[2] == 0 and got[4] == 0 and got[3] == dy[3] and got[5] == dy[5]     # one step outside / inside
    else:
        assert got[2] == 0 and got[3] == 0 and got[4] == 0 and got[5] == 0


@pytest.mark.parametrize("last", ["empty", "full", None])
@pytest.mark.parametrize("rows", [1, 7, 40])
def test_pooling_weight_references_equal_embedding_bag_autograd(last, rows):
    """ragged bags with empty ones, the last bag empty / not, a single-row table (every lookup collides) and rows hit many times in and across bags"""
    rng = np.random.default_rng(5 + rows)
    B, D = 37, 6
    off, idx = ragged_bags(rng, B, rows, 5, last=last)
    if idx.size >= 4 and rows > 1:
        idx[:3] = 2                                                    # one row three times in the first non-empty bag ...
        idx[-1] = 2                                                    # ... and again in the last one
    W = rng.standard_normal((rows, D)).astype(np.float32)
    vW = rng.standard_normal(rows).astype(np.float32)
    dout = rng.standard_normal((B, D)).astype(np.float32)
    psw = psw_gather_ref(vW, idx)
    tv = torch.from_numpy(vW).double().requires_grad_(True)
    ti = torch.from_numpy(idx)
    tpsw = tv[ti]
    assert np.array_equal(psw.astype(np.float64), tpsw.detach().numpy())
    out = Fn.embedding_bag(ti, torch.from_numpy(W).double(), torch.from_numpy(off), per_sample_weights=tpsw, mode="sum")
    out.backward(torch.from_numpy(dout).double())
    dvW, c, S = psw_grad_ref(W, idx, off, dout)
    np.testing.assert_allclose(dvW, tv.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert np.array_equal(c, np.bincount(idx, minlength=rows)) and np.all(dvW[c == 0] == 0) and np.all(S >= np.abs(dvW) - 1e-12)
    assert bag_of_lookup(off, idx.size).size == idx.size
    if last == "empty":
        assert off[-1] == idx.size
    if last == "full":
        assert bag_of_lookup(off, idx.size)[-1] == B - 1


def test_bf16_rounding_restatement_at_ties_and_overflow():
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,      # ties to even (down, up), next to a tie, negative
                     0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000,                  # last value that stays finite; first that overflows
                     0x00000000, 0x80000000, 0x00008000, 0x00018000, 0x7F800000], dtype=np.uint32)
    x = bits.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16)
    got = round_nearest(x)
    assert np.array_equal(got, want.view(torch.int16).numpy().view(np.uint16))
    assert list(got[:6]) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0xBF80, 0xBF82]
    assert list(got[6:11]) == [0x7F7F, 0x7F80, 0x7F80, 0xFF7F, 0xFF80]
    assert np.array_equal(bf16_to_f32(got), want.float().numpy())                                  # the widening is torch's, bit for bit
    assert np.array_equal(round_nearest(bf16_to_f32(got)), got)                                    # and rounding a widened value gives it back
