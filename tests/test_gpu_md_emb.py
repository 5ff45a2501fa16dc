"""Mixed-dimension (MD) embedding tables on the device: dlrm_emb_fwd_md / dlrm_emb_md_bwd (csrc/emb_md.hip), the existing sparse updates over
the width groups, and DLRM_Net(md_flag=True) against the live reference's training run (tests/golden/md_training.npz).

Bars (derived, not tuned):
  * `saved` (the pooled sums) and the output of identity tables: bit-identical to torch's CPU F.embedding_bag(mode="sum") / to ops.emb_fwd;
  * a projected output: within (d + 1) * 2^-23 * sum_c |pooled_c * P_jc| of the float64 product of the fp32 pooled values — the first-order
    bound of a d-term fma chain (d roundings of 2^-24 relative each) with a factor-2 margin;  gout: the same over D terms;
  * dproj: within (B + 1) * 2^-23 * sum_b |dout * pooled| of float64;
  * the deterministic update through the width groups: bit-exact against torch's sparse step; SORTED / ATOMIC rtol 1e-5 / atol 2e-5;
  * the model: loss 1e-5 relative, predictions rtol 2e-5 / atol 1e-6, parameters rtol 1e-4 / atol 2e-6 against the live reference.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_md_emb_host as H
from conftest import ROOT, load_golden, params_with_prefix

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -23
WORST = {}                 # measured error / bound, printed by the tests (docs/PARITY.md quotes them)


def dev():
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def dev_tensor(a: np.ndarray, aligned=True):
    """a copy of `a` on the device; aligned=False: its first element sits 4 bytes past a 16-byte boundary"""
    if aligned:
        return to_dev(a)
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=dev())
    v = flat[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4
    return v


def canary(B, width, ld, c0=0):
    """a [B, width] view inside a NaN-filled [(B + 2), ld] buffer (one row above, one below, columns left and right)"""
    full = torch.full((B + 2, ld), float("nan"), dtype=torch.float32, device=dev())
    return full, full[1:B + 1, c0:c0 + width]


def outside_is_nan(full, B, c0, width, holes=()):
    m = torch.ones_like(full, dtype=torch.bool)
    m[1:B + 1, c0:c0 + width] = False
    for a, b in holes:                                           # columns inside the view nobody writes (padding between width groups)
        m[1:B + 1, c0 + a:c0 + b] = True
    return bool(torch.isnan(full[m]).all())


def make_case(seed, D, dims, rows, B, kinds):
    rng = np.random.default_rng(seed)
    W = [rng.uniform(-1, 1, size=(n, d)).astype(np.float32) for n, d in zip(rows, dims)]
    P = [None if d == D else rng.uniform(-1, 1, size=(D, d)).astype(np.float32) for d in dims]
    offs, idxs = zip(*[H.make_bags(rng, n, B, k) for n, k in zip(rows, kinds)])
    return W, P, list(offs), list(idxs)


def check_forward(D, dims, rows, B, kinds, idx_dtype=torch.int64, wide=False, aligned=True, seed=0, sample=None):
    """one dlrm_emb_fwd_md launch against torch's CPU embedding_bag (saved: bits) and the float64 product (out: the fma-chain bound)"""
    from dlrm_amd import ops
    T = len(dims)
    W, P, offs, idxs = make_case(seed, D, dims, rows, B, kinds)
    dW = [dev_tensor(w, aligned) for w in W]
    dP = [None if p is None else dev_tensor(p, aligned) for p in P]
    bags = ops.BagBatch([to_dev(o, idx_dtype) for o in offs], [to_dev(i, idx_dtype) for i in idxs])
    lay = ops.MDLayout(dims)
    shift = 0 if aligned else 1
    ld, c0 = ((1 + T) * D + 8, D + shift) if wide else (T * D + shift, shift)
    full, out = canary(B, T * D, ld, c0)
    sfull, saved = canary(B, lay.width, lay.width + 4 + shift, shift)
    ops.emb_fwd_md(dW, dP, D, bags, out, saved, lay.cols)
    ops.check_index_errors(sync=True)
    got, got_saved = out.cpu().numpy(), saved.cpu().numpy()
    holes = [(c + len(ks) * d, (c + len(ks) * d + 3) // 4 * 4) for d, ks, c in lay.groups]
    assert outside_is_nan(full, B, c0, T * D), "the lookup wrote outside out"
    assert outside_is_nan(sfull, B, shift, lay.width, holes), "the lookup wrote outside its columns of saved"
    full2, out2 = canary(B, T * D, ld, c0)
    ops.emb_fwd_md(dW, dP, D, bags, out2, None, None)                     # second run, without saved: the same bits
    assert torch.equal(out, out2)
    ident = [t for t in range(T) if P[t] is None]
    if ident:
        ref_out = torch.empty((B, len(ident) * D), device=dev())
        ops.emb_fwd([to_dev(W[t]) for t in ident], ops.bag_subset(bags, ident), ref_out)
        ref_out = ref_out.cpu().numpy()
    rs = slice(None) if sample is None else sample
    worst = 0.0
    for t in range(T):
        pooled = H.torch_pooled(W[t], idxs[t], offs[t])
        assert np.array_equal(got_saved[:, lay.cols[t]:lay.cols[t] + dims[t]].view(np.uint32), pooled.view(np.uint32)), "saved, table %d" % t
        o = got[:, t * D:(t + 1) * D]
        if P[t] is None:
            assert np.array_equal(o.view(np.uint32), pooled.view(np.uint32)), "identity table %d" % t
            k = ident.index(t)
            assert np.array_equal(o.view(np.uint32), ref_out[:, k * D:(k + 1) * D].view(np.uint32)), "identity table %d vs emb_fwd" % t
            continue
        p64, P64 = pooled[rs].astype(np.float64), P[t].astype(np.float64)
        want = p64 @ P64.T
        bound = (dims[t] + 1) * EPS * (np.abs(p64) @ np.abs(P64).T)
        err = np.abs(o[rs].astype(np.float64) - want)
        assert (err <= bound).all(), "table %d (d = %d): worst error / bound %.3f" % (t, dims[t], float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
        if kinds[t] == "empty":
            assert (o == 0).all()
    WORST["out"] = max(WORST.get("out", 0.0), worst)
    print("emb_fwd_md D=%d dims=%s B=%d: worst error / bound %.4f" % (D, dims, B, worst))
    return W, P, offs, idxs, got, got_saved


MIXED_DIMS = {8: [1, 8, 2, 3, 4, 8], 12: [12, 1, 3, 4, 8, 2], 16: [8, 16, 4, 4, 4, 1, 12, 3, 2], 64: [32, 64, 1, 12, 2, 8, 64],
              128: [32, 128, 8, 1, 2, 64, 3, 12, 4, 128], 512: [128, 512, 4, 1, 64]}
KINDS = ["ragged", "short", "onehot", "empty", "short", "ragged", "onehot", "short", "ragged", "short"]
ROWS = [1000, 3, 501, 77, 20000, 60, 4, 250, 1200, 9]


@pytest.mark.parametrize("D", sorted(MIXED_DIMS))
@pytest.mark.parametrize("B", [1, 3, 64, 1000])
def test_lookup_mixed_widths(D, B):
    """every width of the issue's list beside identity tables; D = 512 with d = 128 and d = 64 keeps the projection in global memory"""
    dims = MIXED_DIMS[D]
    check_forward(D, dims, ROWS[:len(dims)], B, KINDS[:len(dims)], wide=(B == 64), seed=D + B)


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("wide", [False, True])
def test_lookup_index_width_and_both_output_pitches(idx_dtype, wide):
    check_forward(128, [32, 128, 8, 1, 2], [1000, 3, 501, 77, 20000], 193, ["ragged", "short", "onehot", "empty", "short"], idx_dtype, wide, seed=5)


@pytest.mark.parametrize("D,dims", [(16, [8, 16, 4, 1]), (7, [7, 3, 1, 4]), (128, [32, 128, 4])])
def test_lookup_unaligned_operands(D, dims):
    check_forward(D, dims, [1000, 33, 501, 77][:len(dims)], 130, ["ragged", "short", "onehot", "short"][:len(dims)], aligned=False, seed=D)


def test_lookup_35_tables_two_launch_groups():
    dims = ([16, 8, 4, 2, 1, 3, 12] * 5)
    check_forward(16, dims, [50 + 13 * k for k in range(35)], 70, (["short", "onehot", "ragged"] * 12)[:35], seed=35)


CRITEO_LIKE_ROWS = [2000000, 39043, 17289, 7420, 20263, 3, 7120, 1543, 63, 2000000, 2000000, 403346, 10, 2208, 11938, 155, 4, 976, 14, 2000000,
                    2000000, 2000000, 585935, 12972, 108, 36]


def test_lookup_26_tables_at_batch_65536_with_terabyte_dims():
    """B = 65536, one lookup per bag, D = 128, the Criteo-Terabyte dimensions of md_solver(alpha = 0.3) (tables capped at 2 M rows: the lookup does
    not depend on rows it does not name).  `saved` is compared in full, the projected outputs on 4096 of the rows (the float64 product is host work)"""
    dims = H.TB_DIMS[(0.3, True)]
    sample = np.r_[0:1024, 30000:31024, 64512:65536, np.arange(1024, 65536, 61)[:1024]]
    check_forward(128, dims, CRITEO_LIKE_ROWS, 65536, ["onehot"] * 26, torch.int32, wide=True, seed=26, sample=sample)


def test_a_row_has_the_same_bits_whatever_the_launch():
    from dlrm_amd import ops
    D, dims, rows = 128, [32, 128, 8, 3], [1000, 30, 501, 77]
    W, P, offs, idxs, got, _ = check_forward(D, dims, rows, 1000, ["ragged", "short", "short", "ragged"], seed=9)
    dW, dP = [to_dev(w) for w in W], [None if p is None else to_dev(p) for p in P]
    for b in (0, 517, 999):
        o1, i1 = [], []
        for off, idx in zip(offs, idxs):
            e = off[b + 1] if b + 1 < len(off) else len(idx)
            o1.append(to_dev(np.zeros(1, dtype=np.int64)))
            i1.append(to_dev(idx[off[b]:e]))
        one = torch.empty((1, len(dims) * D), device=dev())
        ops.emb_fwd_md(dW, dP, D, ops.BagBatch(o1, i1), one)
        assert np.array_equal(one.cpu().numpy().view(np.uint32), got[b:b + 1].view(np.uint32)), b


@pytest.mark.parametrize("D,dims", [(128, [32, 128, 1]), (12, [3, 12, 4])])
def test_out_of_range_id_is_skipped_and_reported(D, dims):
    from dlrm_amd import ops
    rows, B = [100, 30, 50], 40
    W, P, offs, idxs = make_case(3, D, dims, rows, B, ["short", "short", "onehot"])
    bad = idxs[0].copy()
    pos = len(bad) // 2
    bad[pos] = rows[0] + 5
    ops.check_index_errors(sync=True)
    bags = ops.BagBatch([to_dev(o) for o in offs], [to_dev(bad)] + [to_dev(i) for i in idxs[1:]])
    out = torch.empty((B, 3 * D), device=dev())
    saved = torch.empty((B, ops.MDLayout(dims).width), device=dev())
    ops.emb_fwd_md([to_dev(w) for w in W], [None if p is None else to_dev(p) for p in P], D, bags, out, saved, ops.MDLayout(dims).cols)
    with pytest.raises(IndexError, match="table 0, index %d, rows %d" % (rows[0] + 5, rows[0])):
        ops.check_index_errors(sync=True)
    keep = np.ones(len(bad), dtype=bool)
    keep[pos] = False
    bag = H.bag_of(offs[0], len(bad))
    want = np.zeros((B, dims[0]), dtype=np.float32)
    for i in np.nonzero(keep)[0]:
        want[bag[i]] += W[0][bad[i]]
    c = ops.MDLayout(dims).cols[0]
    assert np.array_equal(saved.cpu().numpy()[:, c:c + dims[0]].view(np.uint32), want.view(np.uint32))


def test_operators_refuse_wrong_operands():
    from dlrm_amd import ops
    W, P, offs, idxs = make_case(4, 16, [4, 16], [50, 60], 8, ["short", "short"])
    bags = ops.BagBatch([to_dev(o) for o in offs], [to_dev(i) for i in idxs])
    out = torch.empty((8, 32), device=dev())
    with pytest.raises(RuntimeError, match="must have the common width 16"):
        ops.emb_fwd_md([to_dev(W[0]), to_dev(W[1])], [None, None], 16, bags, out)
    with pytest.raises(RuntimeError, match=r"contiguous \[16, 4\] tensor"):
        ops.emb_fwd_md([to_dev(W[0]), to_dev(W[1])], [to_dev(P[0].T.copy()), None], 16, bags, out)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.emb_fwd_md([to_dev(W[0]), to_dev(W[1])], [to_dev(P[0]), None], 16, bags, out[:, :20])
    with pytest.raises(RuntimeError, match="pooled sums were not kept"):
        ops.emb_md_bwd([to_dev(P[0]), None], [4, 16], 16, out, None, [16, 0], torch.empty((8, 20), device=dev()))


# ------------------------------------------------------------------------------------------------ backward
def check_backward(D, dims, B, aligned=True, seed=0):
    from dlrm_amd import ops
    T = len(dims)
    rng = np.random.default_rng(seed)
    P = [None if d == D else rng.uniform(-1, 1, size=(D, d)).astype(np.float32) for d in dims]
    lay = ops.MDLayout(dims)
    shift = 0 if aligned else 1
    dout = rng.standard_normal((B, T * D)).astype(np.float32)
    pooled = rng.standard_normal((B, lay.width)).astype(np.float32)
    dfull, ddout = canary(B, T * D, T * D + 4 + shift, shift)
    ddout.copy_(torch.from_numpy(dout))
    sfull, dsaved = canary(B, lay.width, lay.width + shift, shift)
    dsaved.copy_(torch.from_numpy(pooled))
    gfull, gout = canary(B, lay.width, lay.width + 8 + shift, 4 + shift)
    dP = [None if p is None else dev_tensor(p, aligned) for p in P]
    _, dproj = ops.emb_md_bwd(dP, dims, D, ddout, dsaved, lay.cols, gout)
    torch.cuda.synchronize()
    holes = [(c + len(ks) * d, (c + len(ks) * d + 3) // 4 * 4) for d, ks, c in lay.groups]
    assert outside_is_nan(gfull, B, 4 + shift, lay.width, holes), "the backward wrote outside its columns of gout"
    g = gout.cpu().numpy()
    _, dproj2 = ops.emb_md_bwd(dP, dims, D, ddout, dsaved, lay.cols, torch.empty_like(gout))
    wg = wp = 0.0
    for t in range(T):
        c, d = lay.cols[t], dims[t]
        do = dout[:, t * D:(t + 1) * D]
        if P[t] is None:
            assert dproj[t] is None
            assert np.array_equal(g[:, c:c + d].view(np.uint32), do.view(np.uint32)), "identity table %d: gout is a copy" % t
            continue
        do64, P64, s64 = do.astype(np.float64), P[t].astype(np.float64), pooled[:, c:c + d].astype(np.float64)
        err = np.abs(g[:, c:c + d] - do64 @ P64)
        bound = (D + 1) * EPS * (np.abs(do64) @ np.abs(P64))
        assert (err <= bound).all(), "gout, table %d: worst error / bound %.3f" % (t, float((err / bound).max()))
        wg = max(wg, float((err / bound).max()))
        assert torch.equal(dproj[t], dproj2[t]), "dproj of table %d differs between two runs" % t
        err = np.abs(dproj[t].cpu().numpy() - do64.T @ s64)
        bound = (B + 1) * EPS * (np.abs(do64).T @ np.abs(s64))
        assert (err <= bound).all(), "dproj, table %d: worst error / bound %.3f" % (t, float((err / bound).max()))
        wp = max(wp, float((err / bound).max()))
    WORST["gout"], WORST["dproj"] = max(WORST.get("gout", 0.0), wg), max(WORST.get("dproj", 0.0), wp)
    print("emb_md_bwd D=%d dims=%s B=%d: worst error / bound  gout %.4f  dproj %.4f" % (D, dims, B, wg, wp))


@pytest.mark.parametrize("D", sorted(MIXED_DIMS))
@pytest.mark.parametrize("B", [1, 3, 64, 1000])
def test_backward_mixed_widths(D, B):
    """B = 1000: two slabs of dproj partials, the second one short"""
    check_backward(D, MIXED_DIMS[D], B, seed=D + B)


@pytest.mark.parametrize("D,dims", [(16, [8, 16, 4, 1]), (7, [7, 3, 1, 4])])
def test_backward_unaligned_operands(D, dims):
    check_backward(D, dims, 130, aligned=False, seed=D)


def test_backward_at_batch_65536():
    """128 slabs of dproj partials; every power-of-two width of the Terabyte dimensions in one call"""
    check_backward(128, [1, 2, 4, 8, 16, 32, 64, 128], 65536, seed=65536)


def test_backward_35_tables_two_launch_groups():
    check_backward(16, [16, 8, 4, 2, 1, 3, 12] * 5, 600, seed=35)


# ------------------------------------------------------------------------------------------------ updates through the width groups
UPD_DIMS = [1, 2, 3, 4, 32, 32, 4, 1]
UPD_ROWS = [4, 3, 5, 4, 6, 200003, 40, 100000]       # the small ones: thousands of duplicates per row; the large ones: most rows untouched


def update_case(seed, B=4096):
    D = 32
    W, P, offs, idxs = make_case(seed, D, UPD_DIMS, UPD_ROWS, B, ["short", "onehot", "short", "short", "short", "short", "onehot", "short"])
    rng = np.random.default_rng(seed + 1)
    dout = (rng.standard_normal((B, len(UPD_DIMS) * D)) * 0.1).astype(np.float32)
    return D, W, P, offs, idxs, dout


def device_step(mode, case, lr, idx_dtype=torch.int64):
    """forward (keeps the sums) -> emb_md_bwd -> one sparse SGD step per width group over a column view of gout.  Returns the tables and gout"""
    from dlrm_amd import ops
    D, W, P, offs, idxs, dout = case
    dims = [w.shape[1] for w in W]
    dW, dP = [to_dev(w) for w in W], [None if p is None else to_dev(p) for p in P]
    bags = ops.BagBatch([to_dev(o, idx_dtype) for o in offs], [to_dev(i, idx_dtype) for i in idxs])
    lay = ops.MDLayout(dims)
    B = len(offs[0])
    out = torch.empty((B, len(dims) * D), device=dev())
    saved = torch.empty((B, lay.width), device=dev())
    ops.emb_fwd_md(dW, dP, D, bags, out, saved, lay.cols)
    gout = torch.empty((B, lay.width), device=dev())
    ops.emb_md_bwd(dP, dims, D, to_dev(dout), saved, lay.cols, gout)
    g = gout.cpu().numpy().copy()
    assert len(lay.groups) == 5
    for d, ks, c0 in lay.groups:
        ops.emb_bwd_sgd([dW[k] for k in ks], ops.bag_subset(bags, ks), gout[:, c0:c0 + len(ks) * d], lr, mode)
    ops.check_index_errors(sync=True)
    return [w.cpu().numpy() for w in dW], g, lay


def torch_sparse_step(case, g, lay, lr):
    """the reference's step per table: the uncoalesced sparse COO gradient (indices verbatim, values = the gradient rows of the pooled sums)
    consumed by torch.optim.SGD on the CPU"""
    _, W, _, offs, idxs, _ = case
    res = []
    for t, (w, off, idx) in enumerate(zip(W, offs, idxs)):
        vals = g[:, lay.cols[t]:lay.cols[t] + w.shape[1]][H.bag_of(off, len(idx))]
        p = torch.nn.Parameter(torch.from_numpy(w.copy()))
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(idx).reshape(1, -1), torch.from_numpy(np.ascontiguousarray(vals)), size=w.shape)
        torch.optim.SGD([p], lr=lr).step()
        res.append((p.detach().numpy(), np.bincount(idx, minlength=w.shape[0])))
    return res


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_deterministic_update_is_bit_exact_against_the_torch_sparse_step(idx_dtype):
    from dlrm_amd import ops
    case = update_case(11)
    got, g, lay = device_step(ops.UPD_DETERMINISTIC, case, 0.3, idx_dtype)
    want = torch_sparse_step(case, g, lay, 0.3)
    assert min(int(c.max()) for (_, c), n in zip(want, UPD_ROWS) if n < 10) > 1000
    for t, (a, (w, _)) in enumerate(zip(got, want)):
        assert np.array_equal(a.view(np.uint32), w.view(np.uint32)), "table %d (d = %d)" % (t, UPD_DIMS[t])


@pytest.mark.parametrize("mode_name", ["sorted", "atomic"])
def test_fast_updates_meet_their_contract_and_leave_other_rows_alone(mode_name):
    """SORTED / ATOMIC re-associate the sums of duplicate rows: the tolerance of tests/test_gpu_kernels.py (rtol 1e-5, atol 2e-5)"""
    from dlrm_amd import ops
    case = update_case(12)
    got, g, lay = device_step(ops.UPD_SORTED if mode_name == "sorted" else ops.UPD_ATOMIC, case, 0.05)
    want = torch_sparse_step(case, g, lay, 0.05)
    for t, (a, (w, count), s) in enumerate(zip(got, want, case[1])):
        np.testing.assert_allclose(a, w, rtol=1e-5, atol=2e-5, err_msg="table %d (d = %d)" % (t, UPD_DIMS[t]))
        assert np.array_equal(a[count == 0], s[count == 0]), "table %d: an untouched row changed" % t
    assert any((c == 0).any() for _, c in want)


# ------------------------------------------------------------------------------------------------ model against the live reference
def batch_to_dev(X, lS_o, lS_i, T, idx_dtype=torch.int64):
    return to_dev(X), [to_dev(o, idx_dtype) for o in lS_o], [to_dev(i, idx_dtype) for i in lS_i], to_dev(T)


def train_and_check(name, configure, make_opt=None, idx_dtype=torch.int64):
    from dlrm_amd import ops
    d, meta = load_golden("md_training")
    case = meta["cases"][name]
    model = H.build_md_model(case, meta["md_threshold"], params=params_with_prefix(d, name + ".init"), seed=1).to(dev())
    configure(model)
    opt = (make_opt or (lambda ps: torch.optim.SGD(ps, lr=meta["lr"])))(model.parameters())
    preds = []
    for s, batch in enumerate(H.case_batches(d, name, case, meta["steps"])):
        X, lS_o, lS_i, T = batch_to_dev(*batch, idx_dtype=idx_dtype)
        Z = model(X, lS_o, lS_i)
        E = model.loss_fn(Z, T)
        opt.zero_grad()
        E.backward()
        opt.step()
        ops.check_index_errors(sync=True)
        want_loss = float(d[f"{name}.s{s}.loss"])
        print("%s step %d: loss %.8f (reference %.8f)" % (name, s, float(E), want_loss))
        np.testing.assert_allclose(Z.detach().cpu().numpy(), d[f"{name}.s{s}.pred"], rtol=2e-5, atol=1e-6, err_msg="predictions, step %d" % s)
        assert abs(float(E) - want_loss) <= 1e-5 * abs(want_loss), "loss, step %d" % s
        preds.append(Z.detach().clone())
    final = params_with_prefix(d, name + ".final")
    sd = model.state_dict()
    assert list(sd) == list(final)
    for k, v in final.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v, rtol=1e-4, atol=2e-6, err_msg=k)
    assert not model._pending_emb
    return model, d, meta, preds


@pytest.mark.parametrize("name", H.CASES)
@pytest.mark.parametrize("mode_name", ["sorted", "atomic", "deterministic"])
def test_model_trains_like_the_live_reference(name, mode_name):
    from dlrm_amd import ops
    mode = {"sorted": ops.UPD_SORTED, "atomic": ops.UPD_ATOMIC, "deterministic": ops.UPD_DETERMINISTIC}[mode_name]
    train_and_check(name, lambda m: setattr(m, "emb_update_mode", mode), idx_dtype=torch.int32 if mode_name == "atomic" else torch.int64)


@pytest.mark.parametrize("name", H.CASES)
def test_model_trains_with_sparse_coo_gradients_and_torch_sgd(name):
    """fused_emb_update = False: embs.weight.grad is the reference's sparse COO gradient, proj.weight.grad is dense, torch.optim.SGD consumes both"""
    def configure(m):
        m.fused_emb_update = False
    model, _, _, _ = train_and_check(name, configure)
    assert all(e.embs.weight.grad is not None and e.embs.weight.grad.is_sparse for e in model.emb_l)
    projs = [e.proj.weight for e in model.emb_l if isinstance(e.proj, torch.nn.Linear)]
    assert len(projs) >= 2 and all(p.grad is not None and not p.grad.is_sparse for p in projs)


def test_model_trains_with_fused_sgd():
    from dlrm_amd.optim import FusedSGD
    train_and_check("pow2", lambda m: None, make_opt=lambda ps: FusedSGD(ps, lr=0.1))


def test_overlap_streams_and_update_in_backward_give_the_same_bits():
    """deterministic update: the side-stream schedule, and update_in_backward (which falls back to the step-time update), change no bit"""
    from dlrm_amd import ops

    def base(m):
        m.emb_update_mode = ops.UPD_DETERMINISTIC
    ref_model, _, _, ref_preds = train_and_check("odd", base)
    for attr in ("overlap_streams", "update_in_backward"):
        def configure(m):
            base(m)
            setattr(m, attr, True)
        model, _, _, preds = train_and_check("odd", configure)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(preds, ref_preds)), attr
        sa, sb = model.state_dict(), ref_model.state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa), attr


def test_evaluate_inference_on_a_trained_md_model():
    """evaluate.inference on the trained model: its metrics are dlrm_binary_metrics of the model's own predictions, and those predictions are
    the torch CPU composition's from the trained parameters at the prediction tolerance"""
    from dlrm_amd import evaluate, ops
    model, d, meta, _ = train_and_check("pow2", lambda m: None)
    case = meta["cases"]["pow2"]
    tm = H.TorchMDModel({k: v.cpu().numpy() for k, v in model.state_dict().items()}, case)
    batches, own, targets = [], [], []
    for X, lS_o, lS_i, T in H.case_batches(d, "pow2", case, meta["steps"]):
        batches.append((torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i], torch.from_numpy(T)))
        with torch.no_grad():
            Z = model(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])
            np.testing.assert_allclose(Z.cpu().numpy(), tm.forward(X, lS_o, lS_i).detach().numpy(), rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
        own.append(Z.reshape(-1))
        targets.append(T)
    got = evaluate.inference(model, batches, device=dev())
    want = ops.binary_metrics(torch.cat(own).contiguous(), to_dev(np.concatenate(targets).reshape(-1)))
    assert got["n"] == sum(len(t) for t in targets)
    assert got == want


def test_apply_emb_keeps_the_reference_shape_and_the_holder_works_alone():
    d, meta = load_golden("md_training")
    case = meta["cases"]["odd"]
    params = params_with_prefix(d, "odd.init")
    model = H.build_md_model(case, meta["md_threshold"], params=params, seed=1).to(dev())
    X, lS_o, lS_i, _ = H.case_batches(d, "odd", case, 1)[0]
    with torch.no_grad():
        ly = model.apply_emb([to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i], model.emb_l, model.v_W_l)
    assert len(ly) == len(case["ln_emb"]) and all(tuple(v.shape) == (X.shape[0], 16) for v in ly)
    for k in range(len(ly)):
        pooled = H.torch_pooled(params[f"emb_l.{k}.embs.weight"], lS_i[k], lS_o[k])
        if f"emb_l.{k}.proj.weight" not in params:
            assert np.array_equal(ly[k].cpu().numpy(), pooled), k
        one = model.emb_l[k](to_dev(lS_i[k]), to_dev(lS_o[k]))          # the holder on its own: forward-only, no autograd node
        assert torch.equal(one, ly[k]) and one.grad_fn is None and not one.requires_grad


def test_a_table_at_or_below_the_threshold_trains_as_a_plain_table():
    """md_flag with tables on both sides of the threshold: plain [n, base] tables ride the MD lookup as identity tables; training follows the
    torch-operator composition at the project's bars"""
    from dlrm_amd import ops
    case = {"ln_emb": [300, 3, 40, 200], "ln_bot": [13, 8], "ln_top": [8 + 10, 1], "sigmoid_top": 0}
    model = H.build_md_model(case, 100, dims=[2, 8, 4, 3], seed=3)
    tm = H.TorchMDModel({k: v.numpy() for k, v in model.state_dict().items()}, case)
    model = model.to(dev())
    model.emb_update_mode = ops.UPD_DETERMINISTIC
    opt, topt = torch.optim.SGD(model.parameters(), lr=0.1), torch.optim.SGD(list(tm.p.values()), lr=0.1)
    rng = np.random.default_rng(8)
    for s in range(2):
        X, T = rng.random((50, 13)).astype(np.float32), np.round(rng.random((50, 1))).astype(np.float32)
        lS_o, lS_i = zip(*[H.make_bags(rng, n, 50, "short") for n in case["ln_emb"]])
        dX, dO, dI, dT = batch_to_dev(X, lS_o, lS_i, T)
        Z = model(dX, dO, dI)
        E = model.loss_fn(Z, dT)
        opt.zero_grad()
        E.backward()
        opt.step()
        loss, pred = tm.train_step(topt, X, lS_o, lS_i, T)
        np.testing.assert_allclose(Z.detach().cpu().numpy(), pred, rtol=2e-5, atol=1e-6)
        assert abs(float(E) - loss) <= 1e-5 * abs(loss)
    for k, v in tm.state().items():
        np.testing.assert_allclose(model.state_dict()[k].cpu().numpy(), v, rtol=1e-4, atol=2e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ launcher
def _reference_dir() -> str:
    """$DLRM_REFERENCE (a checkout), else oracle/_ref (the reference compiled where it lay; built by __graft_entry__.build())"""
    env = os.environ.get("DLRM_REFERENCE", "")
    if env and os.path.isfile(os.path.join(env, "dlrm_s_pytorch.py")):
        return env
    from oracle.build_ref import ref_dir
    return ref_dir() or ""


_REF = _reference_dir()


@pytest.mark.skipif(not _REF, reason="no reference: neither $DLRM_REFERENCE nor a usable oracle/_ref (run `make -C oracle ref` where a "
                                     "checkout exists)")
def test_launcher_with_md_flag_matches_the_reference_cpu_run(tmp_path):
    """the UNMODIFIED reference CLI with --md-flag: through dlrm_amd.launch on the GPU, and as it is on the CPU — every printed loss at 1e-5
    (identical seeds: identical numpy- and torch-drawn parameters, identical data).  Without --md-round-dims: with it the reference's solver
    returns FLOAT dimensions, which its own nn.EmbeddingBag refuses."""
    cli = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=31-32-1", "--arch-embedding-size=60-3-500-1200-250",
           "--data-generation=random", "--mini-batch-size=64", "--num-batches=8", "--nepochs=1", "--num-indices-per-lookup=3",
           "--print-freq=1", "--print-time", "--numpy-rand-seed=73", "--learning-rate=0.05",
           "--loss-function=bce",            # losses near 0.7, printed with 6 decimals: the print's own 5e-7 is far below the 1e-5 relative bar
           "--md-flag", "--md-threshold=2", "--md-temperature=0.3"]
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    ours = subprocess.run([sys.executable, "-m", "dlrm_amd.launch", "--reference", _REF, "--"] + cli + ["--use-gpu"],
                          cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert ours.returncode == 0, ours.stdout[-1500:] + ours.stderr[-3000:]
    stub = ("import sys, types; tb = types.ModuleType('torch.utils.tensorboard'); "
            "tb.SummaryWriter = type('S', (), {'__init__': lambda s, *a, **k: None, 'add_scalar': lambda s, *a, **k: None, 'close': lambda s: None}); "
            "import torch.utils; sys.modules['torch.utils.tensorboard'] = tb; sys.path.insert(0, %r); sys.argv = ['dlrm_s_pytorch.py'] + %r; "
            "import dlrm_s_pytorch as r; r.run()" % (_REF, cli))
    ref = subprocess.run([sys.executable, "-c", stub], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert ref.returncode == 0, ref.stderr[-3000:]
    pat = re.compile(r"Finished training it (\d+)/\d+ of epoch 0, [\d.]+ ms/it, loss ([\d.]+)")
    lo, lr_ = pat.findall(ours.stdout), pat.findall(ref.stdout)
    print("launcher: ", lo, "\nreference:", lr_)
    assert len(lo) >= 8 and len(lo) == len(lr_), (ours.stdout[-1500:], ref.stdout[-1500:])
    for (i, a), (j, b) in zip(lo, lr_):
        assert i == j and abs(float(a) - float(b)) <= 1e-5 * float(b), (i, a, b)


# ------------------------------------------------------------------------------------------------ refusals on the device
def small_md_model(**kw):
    d, meta = load_golden("md_training")
    case = meta["cases"]["pow2"]
    model = H.build_md_model(case, meta["md_threshold"], params=params_with_prefix(d, "pow2.init"), seed=1, **kw).to(dev())
    return model, batch_to_dev(*H.case_batches(d, "pow2", case, 1)[0])


def test_fused_rwsadagrad_refuses_md_tables():
    from dlrm_amd.optim import FusedRWSAdagrad
    model, (X, lS_o, lS_i, T) = small_md_model()
    opt = FusedRWSAdagrad(model.parameters(), lr=0.01)
    model.loss_fn(model(X, lS_o, lS_i), T).backward()
    with pytest.raises(SystemExit, match="ERROR: the fused row-wise Adagrad update is not built for mixed-dimension embedding tables"):
        opt.step()
    model._pending_emb.clear()


def test_pooling_weights_handed_to_apply_emb_are_refused():
    model, (X, lS_o, lS_i, _) = small_md_model()
    vws = [torch.ones(n, device=dev()) for n in [60, 3, 500, 1200, 250]]
    with pytest.raises(SystemExit, match="ERROR: mixed dimensions with weighted pooling is not supported"):
        model.apply_emb(lS_o, lS_i, model.emb_l, vws)


# ------------------------------------------------------------------------------------------------ no regression
@pytest.mark.parametrize("fixture", ["config1_b128", "lr_schedule_onehot_d128"])
def test_a_model_without_md_tables_gives_the_same_bits_with_and_without_the_flag(fixture):
    """md_flag=False is the default: a model built with the keyword spelled out takes the code it took before — apply_emb and a
    deterministic-mode training step through sequential_forward give the same bits as a model built without it"""
    import dlrm_amd
    from dlrm_amd import ops
    d, meta = load_golden(fixture)
    T = len(meta["ln_emb"])
    results = []
    for kw in ({}, dict(md_flag=False, md_threshold=1), {}):
        np.random.seed(1)
        model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]), "dot",
                                  sigmoid_top=meta["sigmoid_top"], loss_function="bce", **kw)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in params_with_prefix(d, "init").items()})
        model = model.to(dev())
        assert not model._has_md(model.emb_l)
        model.emb_update_mode = ops.UPD_DETERMINISTIC
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        lS_o, lS_i = [to_dev(d[f"s0.off{k}"]) for k in range(T)], [to_dev(d[f"s0.idx{k}"]) for k in range(T)]
        with torch.no_grad():
            ly = torch.cat(model.apply_emb(lS_o, lS_i, model.emb_l, model.v_W_l), dim=1).clone()
        Z = model(to_dev(d["s0.X"]), lS_o, lS_i)
        E = model.loss_fn(Z, to_dev(d["s0.T"]))
        opt.zero_grad()
        E.backward()
        opt.step()
        torch.cuda.synchronize()
        results.append((ly, Z.detach().clone(), {k: v.clone() for k, v in model.state_dict().items()}))
    for ly, Z, sd in results[1:]:
        assert torch.equal(ly, results[0][0]) and torch.equal(Z, results[0][1])
        assert all(torch.equal(sd[k], results[0][2][k]) for k in sd)
