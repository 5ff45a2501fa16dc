"""Every value of the template arguments that the interaction's host dispatch (csrc/interact.hip: plan_fwd / plan_bwd, dispatch_n) can select
is launched once, at the smallest batch that still goes wrong: NI = ceil(F / 2) = 1 .. 16 of the D = 128 LDS-DMA kernels (plain, with the
lookups fused, with the update inside the backward), NB = 1 .. 4 and both staging forms of the generic kernels, each with and without a
launch predicate — and the dynamic-LDS limit of the kernels whose LDS follows the call (csrc/common.h dlrm_lds_limit) is raised in a
process that began with a small one.  B = 9 is more than two passes of a four-wave workgroup: the double buffer wraps.
Only valid ids and one lookup per bag; tests/test_gpu_kernels.py feeds the others."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# the dispatched values (tools/interact_dispatch_identity.py walks the same lists)
PLAIN_F = list(range(1, 33))            # NI = 1 .. 16, each from an odd and an even F
GATHER_F = list(range(2, 28))           # the gather form ends at F = 27 (dlrm_interact_gather_ok)
UPDATE_F = [2, 3, 16, 17, 27]
# D = 16: float4 staging, NB = ceil(F / 16) = 1, 2, 3, 4 of the backward; D = 12: float4 staging of a row that is no power of two; D = 6: scalar staging
GENERIC_SHAPES = [(16, 16), (17, 16), (33, 16), (49, 16), (6, 12), (6, 6)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def width(F, D, mode):
    return D + (F * (F + 1) // 2 if mode & 1 else F * (F - 1) // 2)


def triu_perm(F, D):
    """column j of the torchrec-ordered R (mode 2) is column perm[j] of the reference-ordered one (oracle.OracleDLRM._triu_perm)"""
    return np.asarray(list(range(D)) + [D + b * (b - 1) // 2 + a for a in range(F) for b in range(a + 1, F)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(F, D, B, mode):
    """features, dR and the float64 oracle's R and feature gradients, computed once per shape and never written to"""
    rng = np.random.default_rng(100000 * F + 100 * D + 10 * B + mode)
    feat = rng.standard_normal((B, F, D)).astype(np.float32)
    W = width(F, D, mode)
    dR = rng.standard_normal((B, W)).astype(np.float32)
    if mode == 2:
        perm = triu_perm(F, D)
        want = O.interact_fwd(feat, False)[:, perm]
        d_tril = np.empty_like(dR)
        d_tril[:, perm] = dR
        dwant = O.interact_bwd(feat, d_tril, False)
    else:
        want = O.interact_fwd(feat, bool(mode))
        dwant = O.interact_bwd(feat, dR, bool(mode))
    for a in (feat, dR, want, dwant):
        a.setflags(write=False)
    return feat, dR, want, dwant


def check_plain(F, D, B, mode, pred=None):
    """ops.interact_fwd / interact_bwd against the oracle at the bars of test_gpu_kernels.py::test_interact_fwd_bwd; R's padding columns
    are filled with a sentinel beforehand and must come back zero"""
    from dlrm_amd import ops
    feat, dR, want, dwant = case(F, D, B, mode)
    W = want.shape[1]
    ldr = (W + 3) & ~3
    atol = 1e-5 if B <= 67 else 3e-5
    what = "F=%d D=%d B=%d mode=%d pred=%s" % (F, D, B, mode, pred is not None)
    x = to_dev(feat[:, 0, :])
    E = to_dev(feat[:, 1:, :].reshape(B, (F - 1) * D))
    R = torch.full((B, ldr), 3.0, device=dev())
    ops.interact_fwd([x, E], D, mode, R, pred=pred)
    got = R.cpu().numpy()
    np.testing.assert_allclose(got[:, :W], want, rtol=1e-5, atol=atol, err_msg=what)
    assert np.array_equal(got[:, :D], feat[:, 0, :]), what                  # the copied x block is exact
    assert np.all(got[:, W:] == 0), what
    dRd = torch.zeros((B, ldr), device=dev())
    dRd[:, :W] = to_dev(dR)
    dx = torch.full((B, D), 7.0, device=dev())
    dE = torch.full((B, (F - 1) * D), 7.0, device=dev())
    ops.interact_bwd([x, E], D, mode, dRd, [dx, dE], pred=pred)
    np.testing.assert_allclose(dx.cpu().numpy(), dwant[:, 0, :], rtol=1e-5, atol=2 * atol, err_msg=what)
    np.testing.assert_allclose(dE.cpu().numpy().reshape(B, F - 1, D), dwant[:, 1:, :], rtol=1e-5, atol=2 * atol, err_msg=what)


def check_skipped(F, D, B, mode):
    """a launch behind a predicate that does not hold leaves its outputs as they were"""
    from dlrm_amd import ops
    feat = case(F, D, B, mode)[0]
    ldr = (width(F, D, mode) + 3) & ~3
    x = to_dev(feat[:, 0, :])
    E = to_dev(feat[:, 1:, :].reshape(B, (F - 1) * D))
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    R = torch.full((B, ldr), 3.0, device=dev())
    ops.interact_fwd([x, E], D, mode, R, pred=(flag, 1))
    dx, dE = torch.full((B, D), 7.0, device=dev()), torch.full((B, (F - 1) * D), 7.0, device=dev())
    ops.interact_bwd([x, E], D, mode, torch.ones((B, ldr), device=dev()), [dx, dE], pred=(flag, 1))
    assert bool((R == 3.0).all()) and bool((dx == 7.0).all()) and bool((dE == 7.0).all()), (F, D, B, mode)


# ------------------------------------------------------------------------------------------ D = 128, plain features
@pytest.mark.parametrize("F", PLAIN_F)
def test_every_ni_of_the_plain_image_kernels(F):
    """interact_fwd_dma_kernel<NI, false> / interact_bwd_dma_kernel<NI, false>, NI = ceil(F / 2): every F = 1 .. 32 in the three pair
    orders (0 tril, 1 with the diagonal, 2 torchrec's triu order against the permuted oracle), one sample and nine"""
    for mode in (0, 1, 2):
        for B in (1, 9):
            check_plain(F, 128, B, mode)


# ------------------------------------------------------------------------------------------ D = 128, the lookups fused
def gather_case(F, B, idx_dtype, seed):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    T, D = F - 1, 128
    rows = [int(r) for r in rng.integers(1, 200, size=T)]
    Ws = [to_dev(rng.standard_normal((n, D)).astype(np.float32)) for n in rows]
    idx = torch.stack([to_dev(rng.integers(0, n, size=B)) for n in rows]).to(idx_dtype)
    off = torch.arange(B, device=dev()).repeat(T, 1).to(idx_dtype)
    x = to_dev(rng.standard_normal((B, D)).astype(np.float32))
    return rows, Ws, ops.BagBatch(off, idx), x


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("F", GATHER_F)
def test_every_ni_of_the_gather_image_kernels(F, idx_dtype):
    """interact_fwd_dma_kernel<NI, true> / interact_bwd_dma_kernel<NI, true> for every F = 2 .. 27: the SAME bits as dlrm_emb_fwd + the
    plain kernels (test_gpu_kernels.py::test_gather_interaction_is_bit_identical_to_the_two_kernels), directly, behind a launch predicate
    that says "run" — and behind one that says "skip" nothing is written"""
    from dlrm_amd import ops
    D, T, itself = 128, F - 1, bool(F & 1)
    ldr = (ops.interact_out_width(F, D, itself) + 3) & ~3
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    run, skip = (flag, 0), (flag, 1)
    for B in (1, 9):
        rows, Ws, bags, x = gather_case(F, B, idx_dtype, 1000 * F + B)
        feat = torch.empty((B, F * D), device=dev())
        feat[:, :D] = x
        ops.emb_fwd(Ws, bags, feat[:, D:])
        R0 = torch.full((B, ldr), 5.0, device=dev())
        ops.interact_fwd([feat[:, :D], feat[:, D:]], D, itself, R0)
        for pred in (None, run):
            R1 = torch.full((B, ldr), 7.0, device=dev())
            ops.interact_fwd_gather(x, Ws, bags, D, itself, R1, pred=pred)
            assert torch.equal(R0, R1), (B, pred is not None)
        R2 = torch.full((B, ldr), 7.0, device=dev())
        ops.interact_fwd_gather(x, Ws, bags, D, itself, R2, pred=skip)
        assert bool((R2 == 7.0).all()), B
        dR = torch.randn((B, ldr), device=dev(), generator=torch.Generator(device=dev()).manual_seed(F * 10 + B))
        d0 = torch.empty((B, F * D), device=dev())
        ops.interact_bwd([feat[:, :D], feat[:, D:]], D, itself, dR, [d0[:, :D], d0[:, D:]])
        for pred in (None, run):
            dx, dE = torch.full((B, D), 7.0, device=dev()), torch.full((B, T * D), 7.0, device=dev())
            ops.interact_bwd_gather(x, Ws, bags, D, itself, dR, dx, dE, pred=pred)
            assert torch.equal(d0[:, :D], dx) and torch.equal(d0[:, D:], dE), (B, pred is not None)
        dx, dE = torch.full((B, D), 7.0, device=dev()), torch.full((B, T * D), 7.0, device=dev())
        ops.interact_bwd_gather(x, Ws, bags, D, itself, dR, dx, dE, pred=skip)
        assert bool((dx == 7.0).all()) and bool((dE == 7.0).all()), B
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("F", UPDATE_F)
def test_update_inside_the_backward_at_both_ends_of_ni(F):
    """interact_bwd_dma_kernel<NI, true, true> (presorted=) at NI = 1, 2, 8, 9, 14: what
    test_gpu_kernels.py::test_single_lookup_rows_are_updated_inside_the_fused_backward asserts — the mask against numpy's count of each
    (table, row), the gradient rows of single lookups never written and all others the plain backward's, dx the same bits, the single
    rows already stepped and no other row touched, the tables after the presorted update equal to the two-call route's; behind a predicate
    that does not hold nothing is written or stepped"""
    from dlrm_amd import ops
    T, B, D, itself, lr = F - 1, 9, 128, False, 0.37
    rng = np.random.default_rng(F + 17)
    rows = [max(1, int(B * f)) for f in rng.choice([40.0, 8.0, 1.5, 0.3], size=T)]        # from "every lookup single" to "every row hot"
    rows[0] = max(rows[0], 3)
    gen = torch.Generator(device=dev()); gen.manual_seed(F + 18)
    W0 = [torch.randn((n, D), device=dev(), generator=gen) for n in rows]
    idx = torch.stack([to_dev(rng.integers(0, n, size=B)) for n in rows])
    off = torch.arange(B, device=dev()).repeat(T, 1)
    x = to_dev(rng.standard_normal((B, D)).astype(np.float32))
    bags = ops.BagBatch(off, idx)
    ldr = (ops.interact_out_width(F, D, itself) + 3) & ~3
    dR = to_dev(rng.standard_normal((B, ldr)).astype(np.float32))

    Wa = [w.clone() for w in W0]
    dx_a, dE_a = torch.empty((B, D), device=dev()), torch.empty((B, T * D), device=dev())
    ops.interact_bwd_gather(x, Wa, bags, D, itself, dR, dx_a, dE_a)
    ops.emb_bwd_sgd(Wa, bags, dE_a, lr, ops.UPD_SORTED)

    Wb = [w.clone() for w in W0]
    assert ops.presort_ok(Wb, bags)
    pre = ops.emb_presort(Wb, bags, lr)
    idx_np = idx.cpu().numpy().astype(np.int64)
    counts = [np.bincount(idx_np[t], minlength=rows[t]) for t in range(T)]
    want_mask = np.zeros(B, dtype=np.uint32)
    for t in range(T):
        want_mask |= (counts[t][idx_np[t]] == 1).astype(np.uint32) << np.uint32(t)
    assert np.array_equal(pre.mask.cpu().numpy().view(np.uint32), want_mask)
    once_or_never = [torch.from_numpy(c <= 1).to(dev()) for c in counts]

    def same_tables(Wx):
        # rows looked up at most once: the same bits; hot rows are re-associated by the sorted update in either route (DLRM_UPD_SORTED)
        for t in range(T):
            assert torch.equal(Wa[t][once_or_never[t]], Wx[t][once_or_never[t]]), t
            assert torch.allclose(Wa[t], Wx[t], rtol=1e-5, atol=1e-5), t
    dx_b = torch.empty((B, D), device=dev())
    dE_b = torch.full((B, T * D), float("nan"), device=dev())
    ops.interact_bwd_gather(x, Wb, bags, D, itself, dR, dx_b, dE_b, presorted=pre)
    single = torch.from_numpy(((want_mask[:, None] >> np.arange(T, dtype=np.uint32)[None, :]) & 1).astype(bool)).to(dev())     # [B, T]
    dEb3, dEa3 = dE_b.view(B, T, D), dE_a.view(B, T, D)
    assert torch.isnan(dEb3[single]).all()
    assert torch.equal(dEb3[~single], dEa3[~single])
    assert torch.equal(dx_a, dx_b)
    for t in range(T):
        rows_single = idx[t][single[:, t]].long()
        assert torch.equal(Wb[t][rows_single], Wa[t][rows_single]), t
        keep = torch.ones(rows[t], dtype=torch.bool, device=dev()); keep[rows_single] = False
        assert torch.equal(Wb[t][keep], W0[t][keep]), t
    ops.emb_bwd_sgd_presorted(Wb, bags, dE_b, pre)
    same_tables(Wb)

    flag = torch.ones(1, dtype=torch.int32, device=dev())
    Wc = [w.clone() for w in W0]
    pre_c = ops.emb_presort(Wc, bags, lr, pred=(flag, 0))
    dx_c, dE_c = torch.full((B, D), 3.0, device=dev()), torch.full((B, T * D), 5.0, device=dev())
    ops.interact_bwd_gather(x, Wc, bags, D, itself, dR, dx_c, dE_c, pred=(flag, 0), presorted=pre_c)
    assert bool((dx_c == 3.0).all()) and bool((dE_c == 5.0).all())
    for t in range(T):
        assert torch.equal(Wc[t], W0[t])
    ops.emb_bwd_sgd_presorted(Wc, bags, dE_a, pre_c)
    same_tables(Wc)
    flag.zero_()                                   # ... and one that holds, through the same entry
    Wd = [w.clone() for w in W0]
    pre_d = ops.emb_presort(Wd, bags, lr, pred=(flag, 0))
    dE_d = torch.empty((B, T * D), device=dev())
    ops.interact_bwd_gather(x, Wd, bags, D, itself, dR, dx_c, dE_d, pred=(flag, 0), presorted=pre_d)
    ops.emb_bwd_sgd_presorted(Wd, bags, dE_d, pre_d)
    same_tables(Wd)
    assert torch.equal(dx_a, dx_c)
    ops.check_index_errors(sync=True)


# ------------------------------------------------------------------------------------------ the generic kernels
@pytest.mark.parametrize("F,D", GENERIC_SHAPES)
def test_generic_kernels_with_and_without_a_predicate(F, D):
    """interact_fwd_kernel<PRED> / interact_bwd_kernel<NB, PRED>.  Behind a predicate the grid is capped at 512 workgroups of four samples:
    B = 2052 needs 513, so the kernels' grid stride takes a second pass"""
    mode = 1 if D == 12 else 0
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    check_plain(F, D, 9, mode)
    check_plain(F, D, 9, mode, pred=(flag, 0))
    check_plain(F, D, 2052, mode, pred=(flag, 0))
    check_skipped(F, D, 9, mode)


# ------------------------------------------------------------------------------------------ the dynamic-LDS limit
def tower_check(M, widths, acts):
    """dlrm_tower_fwd / _bwd against the oracle, layer by layer on what the GPU fed each layer (test_small_batch_tower_kernels_match_oracle)"""
    from dlrm_amd import ops
    rng = np.random.default_rng(M + sum(widths))
    L = len(acts)
    X = rng.standard_normal((M, widths[0])).astype(np.float32)
    Ws = [(rng.standard_normal((widths[l + 1], widths[l])) / np.sqrt(widths[l])).astype(np.float32) for l in range(L)]
    bs = [rng.standard_normal(widths[l + 1]).astype(np.float32) for l in range(L)]
    Wd, bd = [to_dev(w) for w in Ws], [to_dev(b) for b in bs]
    outs = [torch.full((M, widths[l + 1]), 7.0, device=dev()) for l in range(L)]
    ops.tower_fwd(to_dev(X), Wd, bd, acts, outs)
    cur = X
    for l in range(L):
        np.testing.assert_allclose(outs[l].cpu().numpy(), O.linear_fwd(cur, Ws[l], bs[l], acts[l]), rtol=1e-5, atol=1e-5,
                                   err_msg="%s layer %d forward" % (widths, l))
        cur = outs[l].cpu().numpy()
    g = rng.standard_normal((M, widths[L])).astype(np.float32)
    dZs = [torch.full((M, widths[l + 1]), 7.0, device=dev()) for l in range(L)]
    dX = torch.full((M, widths[0]), 7.0, device=dev())
    ops.tower_bwd(to_dev(g), Wd, acts, outs, dZs, dX)
    for l in range(L - 1, -1, -1):
        y = outs[l].cpu().numpy().astype(np.float64)
        dz = g * ((y > 0) if acts[l] == 1 else (y * (1 - y)) if acts[l] == 2 else 1.0)
        np.testing.assert_allclose(dZs[l].cpu().numpy(), dz, rtol=1e-5, atol=1e-5, err_msg="%s layer %d dZ" % (widths, l))
        g = (dZs[l].cpu().numpy().astype(np.float64) @ Ws[l].astype(np.float64)).astype(np.float32)
    np.testing.assert_allclose(dX.cpu().numpy(), g, rtol=1e-5, atol=1e-5, err_msg="%s dX" % (widths,))


def lds_limit_sequences():
    """small, large, small — run in a process whose FIRST call of each kernel is the small one"""
    for F in (4, 49, 4):
        check_plain(F, 16, 9, 0)
    for widths in ([8, 8, 4], [64, 512, 64], [8, 8, 4]):
        tower_check(17, widths, [1, 2])
    torch.cuda.synchronize()
    print("lds limit sequences ok")


def test_lds_limit_is_raised_after_a_small_first_call():
    """dlrm_lds_limit remembers the largest dynamic-LDS size it has set per kernel and device.  The generic interaction kernels' LDS follows
    F and D (6 KiB forward and 5 KiB backward at F = 4, D = 16; 21 KiB and 76 KiB at F = 49) and the tower kernels' the widest layer: a
    helper that set the limit once, at the first size, would fail the second call of each sequence.  The order of the calls IS the test,
    so they run in a fresh process — in this one any earlier test may have raised the limits already."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lds limit sequences ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    lds_limit_sequences()
