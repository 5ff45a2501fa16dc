"""Quotient-remainder (QR) embedding tables on the device: dlrm_emb_fwd_qr / dlrm_emb_qr_bwd_split / dlrm_emb_qr_split_indices through
dlrm_amd.ops, the existing sparse updates over the virtual table list, and DLRM_Net(qr_flag=True) forward / training / evaluation.

  * lookup: BIT-IDENTICAL to the reference's composition from torch's CPU operators (two F.embedding_bag(mode="sum") calls, then one multiply
    or add; tests/test_qr_emb_host.py pins the restatements): both are in-order fp32 sums per column followed by one fp32 operation;
  * gradient split: bit-identical to dout * sr, dout * sq, dout;
  * updates: DETERMINISTIC bit-exact against torch's sparse SGD step per component, SORTED / ATOMIC at their documented contracts
    (tests/test_gpu_kernels.py: rtol 1e-5 / atol 2e-5, duplicates re-associated);
  * model: 3 training steps against the live reference (tests/golden/qr_training.npz) at the project's bars — losses 1e-5 relative,
    predictions rtol 2e-5 / atol 1e-6, parameters rtol 1e-4 / atol 2e-6.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_qr_emb_host as H
from conftest import ROOT, load_golden, params_with_prefix

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ forward kernel
def make_tables(rng, rows, coll, D):
    """host tables of a list: (weight or weight_q, weight_r or None) per table"""
    out = []
    for n, c in zip(rows, coll):
        if c:
            out.append((rng.uniform(-1.0, 1.0, size=(H.rows_q(n, c), D)).astype(np.float32), rng.uniform(-1.0, 1.0, size=(c, D)).astype(np.float32)))
        else:
            out.append((rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32), None))
    return out


def torch_cpu_lookup(tables, coll, op, offs, idxs):
    """(out [B, T*D], per QR table (sq, sr)) from torch's CPU operators"""
    cols, sums = [], []
    for (W, Wr), c, off, idx in zip(tables, coll, offs, idxs):
        o, i = torch.from_numpy(off), torch.from_numpy(idx)
        if c:
            sq = F.embedding_bag((i / c).long(), torch.from_numpy(W), o, mode="sum")
            sr = F.embedding_bag(torch.remainder(i, c).long(), torch.from_numpy(Wr), o, mode="sum")
            cols.append(sq * sr if op == "mult" else sq + sr)
            sums.append((sq.numpy(), sr.numpy()))
        else:
            cols.append(F.embedding_bag(i, torch.from_numpy(W), o, mode="sum"))
    return torch.cat(cols, dim=1).numpy(), sums


def run_fwd(D, rows, coll, B, kind, idx_dtype, op, wide, seed, keep_sums=True):
    from dlrm_amd import ops
    rng = np.random.default_rng(seed)
    T = len(rows)
    tables = make_tables(rng, rows, coll, D)
    offs, idxs = zip(*[H.make_bags(rng, n, B, kind) for n in rows])
    bags = ops.BagBatch([to_dev(o, idx_dtype) for o in offs], [to_dev(i, idx_dtype) for i in idxs])
    W = [to_dev(w) for w, _ in tables]
    Wr = [None if r is None else to_dev(r) for _, r in tables]
    CANARY = 7.5
    width = (1 + T) * D if wide else T * D
    buf = torch.full((B, width), CANARY, device=dev())
    out = buf[:, D:] if wide else buf
    nq = sum(1 for c in coll if c)
    saved = torch.full((B, 2 * nq * D + 4), CANARY, device=dev()) if keep_sums else None
    ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, out, None if saved is None else saved[:, :2 * nq * D])
    ops.check_index_errors(sync=True)
    got = buf.cpu().numpy()
    if wide:
        assert (got[:, :D] == CANARY).all(), "columns outside the embedding slots were written"
        got = got[:, D:]
    want, sums = torch_cpu_lookup(tables, coll, op, offs, idxs)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, "%d of %d values differ from the torch CPU composition" % (bad, want.size)
    if keep_sums:
        sv = saved.cpu().numpy()
        assert (sv[:, 2 * nq * D:] == CANARY).all(), "columns beyond the saved sums were written"
        for j, (sq, sr) in enumerate(sums):
            assert np.array_equal(sv[:, 2 * j * D:(2 * j + 1) * D], sq) and np.array_equal(sv[:, (2 * j + 1) * D:(2 * j + 2) * D], sr), j
    # plain tables of the launch: the bits of dlrm_emb_fwd
    plain = [t for t, c in enumerate(coll) if not c]
    if plain:
        ref = torch.empty((B, len(plain) * D), device=dev())
        ops.emb_fwd([W[t] for t in plain], ops.BagBatch([to_dev(offs[t], idx_dtype) for t in plain], [to_dev(idxs[t], idx_dtype) for t in plain]), ref)
        ref = ref.cpu().numpy()
        for j, t in enumerate(plain):
            assert np.array_equal(ref[:, j * D:(j + 1) * D], got[:, t * D:(t + 1) * D]), t
    ends = [np.concatenate([o[1:], [len(i)]]) - o for o, i in zip(offs, idxs)]
    for t in range(T):
        assert (got[:, t * D:(t + 1) * D][ends[t] == 0] == 0).all(), "an empty bag is not zero"


@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("D", [8, 12, 16, 64, 128, 256])
def test_lookup_one_qr_table_ragged(op, D):
    run_fwd(D, [3001], [4], 512, "ragged", torch.int64, op, wide=False, seed=100 + D)          # 3001 = 750 * 4 + 1: a ragged last quotient row


@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["onehot", "ragged", "short", "empty"])
@pytest.mark.parametrize("wide", [False, True])
def test_lookup_five_mixed_tables(op, idx_dtype, kind, wide):
    run_fwd(128, [60, 3, 500, 40001, 250], [0, 0, 7, 4, 60], 1000, kind, idx_dtype, op, wide, seed=200)


@pytest.mark.parametrize("D,wide", [(64, True), (12, True), (12, False), (8, True), (256, False), (512, False)])
def test_lookup_mixed_tables_other_dims(D, wide):
    run_fwd(D, [3, 5000, 100, 977], [0, 4, 3, 1000], 777, "ragged", torch.int32, "mult", wide, seed=300 + D)


CRITEO_LIKE_ROWS = [2000000, 3, 38532, 17289, 7420, 20263, 3, 7120, 1543, 63, 2000000, 976, 14, 100000, 3, 7, 5461, 4, 10, 2208, 4, 7, 122, 3, 305, 36]


@pytest.mark.parametrize("op", ["mult", "add"])
def test_lookup_26_mixed_tables_at_batch_65536(op):
    coll = [4 if n > 200 else 0 for n in CRITEO_LIKE_ROWS]
    run_fwd(128, CRITEO_LIKE_ROWS, coll, 65536, "onehot", torch.int64, op, wide=True, seed=401)


def test_lookup_35_tables_two_launch_groups():
    rows = [(5000 + 37 * k) if k % 3 else (3 + k) for k in range(35)]
    coll = [4 if n > 200 else 0 for n in rows]
    run_fwd(16, rows, coll, 4096, "short", torch.int32, "mult", wide=False, seed=402)
    run_fwd(16, rows, coll, 300, "ragged", torch.int64, "add", wide=True, seed=403, keep_sums=False)


@pytest.mark.parametrize("D", [7, 16])
def test_lookup_unaligned_operands_take_the_scalar_kernel(D):
    """an odd dimension, and a weight_q that is only 4-byte aligned: correct, bit for bit"""
    from dlrm_amd import ops
    rng = np.random.default_rng(17 + D)
    n, c, B = 1001, 4, 300
    (Wq, Wr), = make_tables(rng, [n], [c], D)
    off, idx = H.make_bags(rng, n, B, "short")
    hold = torch.empty(Wq.size + 1, device=dev())
    view = hold[1:].view(Wq.shape)
    view.copy_(to_dev(Wq))
    out = torch.empty((B, D), device=dev())
    saved = torch.empty((B, 2 * D), device=dev())
    ops.emb_fwd_qr([view], [to_dev(Wr)], [n], [c], "mult", ops.BagBatch([to_dev(off)], [to_dev(idx)]), out, saved)
    ops.check_index_errors(sync=True)
    assert np.array_equal(out.cpu().numpy(), H.torch_qr_lookup(Wq, Wr, idx, off, c, "mult"))
    _, sq, sr = H.np_qr_forward(Wq, Wr, idx, off, n, c, "mult")
    assert np.array_equal(saved.cpu().numpy(), np.concatenate([sq, sr], axis=1))


@pytest.mark.parametrize("D", [128, 12])
def test_out_of_range_id_is_skipped_and_reported(D):
    from dlrm_amd import ops
    rng = np.random.default_rng(5)
    rows, coll, B = [501, 60], [4, 0], 300
    tables = make_tables(rng, rows, coll, D)
    offs, idxs = zip(*[H.make_bags(rng, n, B, "short") for n in rows])
    idxs = [i.copy() for i in idxs]
    idxs[0][idxs[0].size // 2] = rows[0]                       # == n: its quotient 125 IS a row of weight_q, the id is still no category
    idxs[0][3] = -1
    idxs[1][5] = rows[1] + 5
    ops.check_index_errors(sync=True)
    out = torch.empty((B, 2 * D), device=dev())
    ops.emb_fwd_qr([to_dev(w) for w, _ in tables], [None if r is None else to_dev(r) for _, r in tables], rows, coll, "mult",
                   ops.BagBatch([to_dev(o) for o in offs], [to_dev(i) for i in idxs]), out)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    got = out.cpu().numpy()
    want, _, _ = H.np_qr_forward(tables[0][0], tables[0][1], idxs[0], offs[0], rows[0], 4, "mult")          # (skips what qr_split refuses)
    assert np.array_equal(got[:, :D], want)
    ops.check_index_errors(sync=True)            # reported once


def test_operators_refuse_wrong_operands():
    from dlrm_amd import ops
    bags = ops.BagBatch([torch.arange(4, device=dev())], [torch.zeros(4, dtype=torch.int64, device=dev())])
    out = torch.empty((4, 16), device=dev())
    Wq, Wr = torch.zeros((25, 16), device=dev()), torch.zeros((4, 16), device=dev())
    with pytest.raises(RuntimeError, match="needs a contiguous weight of shape"):
        ops.emb_fwd_qr([Wq], [Wr], [200], [4], "mult", bags, out)                # 200 categories at 4 collisions are 50 quotient rows
    with pytest.raises(RuntimeError, match="weight_r"):
        ops.emb_fwd_qr([Wq], [Wr[:3]], [100], [4], "mult", bags, out)
    with pytest.raises(RuntimeError, match="'mult' or 'add'"):
        ops.emb_fwd_qr([Wq], [Wr], [100], [4], "concat", bags, out)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.emb_fwd_qr([Wq.cpu()], [Wr], [100], [4], "mult", bags, out)


# ------------------------------------------------------------------------------------------------ a table above 2^24 categories
BIG_N, BIG_C, BIG_D = 40_000_000, 4, 8


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_large_table_rows_follow_the_float32_quotient(idx_dtype):
    """n = 40,000,000, c = 4 (weight_q: 10,000,000 x 8 floats = 320 MB), ids from the top eighth: the rows read are torch's float32 quotient, not
    id // 4; the two ids whose quotient is rows_q are skipped and reported, every other value is the torch CPU composition's"""
    from dlrm_amd import ops
    rng = np.random.default_rng(77)
    B = 16384
    nq = H.rows_q(BIG_N, BIG_C)
    g = torch.Generator(device=dev()).manual_seed(78)
    Wq = torch.rand((nq, BIG_D), device=dev(), generator=g) + 0.5
    Wr = torch.rand((BIG_C, BIG_D), device=dev(), generator=g) + 0.5
    lens = rng.integers(0, 4, size=B)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx = rng.integers(BIG_N - BIG_N // 8, BIG_N, size=int(lens.sum())).astype(np.int64)
    idx[[7, idx.size // 3]] = [39_999_998, 39_999_999]
    q, r, ok = H.qr_split(idx, BIG_N, BIG_C)
    assert np.array_equal(q, (torch.from_numpy(idx) / BIG_C).long().numpy())
    assert int((~ok).sum()) == 2 and int((q != idx // BIG_C).sum()) > idx.size // 8          # the test can tell the two mappings apart
    CANARY = 7.5
    buf = torch.full((B, 2 * BIG_D), CANARY, device=dev())
    before = Wq[-64:].clone()
    ops.check_index_errors(sync=True)
    ops.emb_fwd_qr([Wq], [Wr], [BIG_N], [BIG_C], "mult", ops.BagBatch([to_dev(off, idx_dtype)], [to_dev(idx, idx_dtype)]), buf[:, :BIG_D])
    with pytest.raises(IndexError, match=r"index 3999999[89], rows 40000000"):
        ops.check_index_errors(sync=True)
    # the torch CPU composition over the rows the valid lookups name, re-indexed; the two bad lookups removed from their bags
    uniq, inv = np.unique(q[ok], return_inverse=True)
    small = Wq.index_select(0, to_dev(uniq)).cpu()
    bag = H.bag_of(off, idx.size)[ok]
    off_ok = np.searchsorted(bag, np.arange(B), side="left").astype(np.int64)
    sq = F.embedding_bag(torch.from_numpy(inv.astype(np.int64)), small, torch.from_numpy(off_ok), mode="sum")
    sr = F.embedding_bag(torch.from_numpy(r[ok]), Wr.cpu(), torch.from_numpy(off_ok), mode="sum")
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :BIG_D], (sq * sr).numpy())
    assert (got[:, BIG_D:] == CANARY).all() and torch.equal(before, Wq[-64:])
    # the derived ids of the update: the float quotient, -1 for the two skipped lookups
    qs, rs = ops.emb_qr_split_indices([BIG_N], [BIG_C], ops.BagBatch([to_dev(off, idx_dtype)], [to_dev(idx, idx_dtype)]))
    assert qs[0].dtype == idx_dtype and rs[0].dtype == idx_dtype
    assert np.array_equal(qs[0].cpu().numpy(), np.where(ok, q, -1)) and np.array_equal(rs[0].cpu().numpy(), np.where(ok, r, -1))


# ------------------------------------------------------------------------------------------------ gradient split
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("D,aligned", [(8, True), (12, True), (128, True), (7, True), (16, False)])
def test_backward_split_is_bit_identical(op, D, aligned):
    check_backward_split(op, D, aligned, [0, 4, 0, 7, 4], 1031)


@pytest.mark.parametrize("op", ["mult", "add"])
def test_backward_split_over_two_launch_groups(op):
    """35 and 70 tables: the virtual slot and the saved-sums slot of a table are carried from one launch group of 32 tables into the next"""
    check_backward_split(op, 16, True, [4 if k % 3 else 0 for k in range(35)], 257)
    check_backward_split(op, 8, True, [0 if k % 5 == 1 else 7 for k in range(70)], 64)


def check_backward_split(op, D, aligned, coll, B):
    from dlrm_amd import ops
    rng = np.random.default_rng(900 + D + len(coll))
    T, nq = len(coll), sum(1 for c in coll if c)
    Tv = T + nq
    dout = rng.standard_normal((B, T * D)).astype(np.float32)
    saved = rng.standard_normal((B, 2 * nq * D)).astype(np.float32)
    CANARY = 7.5
    pad = 4 if aligned else 1
    buf = torch.full((B + 1, Tv * D + pad), CANARY, device=dev())
    gout = buf[:B, :Tv * D] if aligned else buf[:B, 1:Tv * D + 1]
    ops.emb_qr_bwd_split(coll, op, D, to_dev(dout), to_dev(saved) if op == "mult" else None, gout)
    torch.cuda.synchronize()
    want, j = [], 0
    for t, c in enumerate(coll):
        g = dout[:, t * D:(t + 1) * D]
        if not c:
            want.append(g)
            continue
        sq, sr = saved[:, 2 * j * D:(2 * j + 1) * D], saved[:, (2 * j + 1) * D:(2 * j + 2) * D]
        want += [g * sr, g * sq] if op == "mult" else [g, g]
        j += 1
    full = np.full((B + 1, Tv * D + pad), CANARY, dtype=np.float32)
    c0 = 0 if aligned else 1
    full[:B, c0:c0 + Tv * D] = np.concatenate(want, axis=1)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:B, c0:c0 + Tv * D].view(np.uint32), full[:B, c0:c0 + Tv * D].view(np.uint32))
    assert np.array_equal(got, full), "the split wrote beyond its buffer"


# ------------------------------------------------------------------------------------------------ updates over the virtual tables
def update_case(seed, D=16, B=4096):
    """one QR table whose 4-row remainder table is named thousands of times per row, one plain table, one QR table with 7 collisions"""
    rng = np.random.default_rng(seed)
    rows, coll = [1001, 40, 200003], [4, 0, 7]            # (the last one: most of its 28572 quotient rows stay untouched)
    tables = make_tables(rng, rows, coll, D)
    offs, idxs = zip(*[H.make_bags(rng, n, B, kind) for n, kind in zip(rows, ["short", "onehot", "short"])])
    dout = (rng.standard_normal((B, len(rows) * D)) * 0.1).astype(np.float32)
    return rows, coll, tables, offs, idxs, dout


def device_step(mode, op, rows, coll, tables, offs, idxs, dout, lr, idx_dtype=torch.int64):
    """forward (keeps the sums) -> gradient split -> virtual bags -> one sparse SGD step; returns the virtual tables"""
    from dlrm_amd import ops
    D = tables[0][0].shape[1]
    W = [to_dev(w) for w, _ in tables]
    Wr = [None if r is None else to_dev(r) for _, r in tables]
    bags = ops.BagBatch([to_dev(o, idx_dtype) for o in offs], [to_dev(i, idx_dtype) for i in idxs])
    B = len(offs[0])
    out = torch.empty((B, len(rows) * D), device=dev())
    saved = torch.empty((B, 2 * D * sum(1 for c in coll if c)), device=dev())
    ops.emb_fwd_qr(W, Wr, rows, coll, op, bags, out, saved)
    gout = ops.emb_qr_bwd_split(coll, op, D, to_dev(dout), saved if op == "mult" else None)
    vb = ops.qr_virtual_bags(rows, coll, bags)
    vw = []
    for w, r in zip(W, Wr):
        vw += [w] if r is None else [w, r]
    assert vb.T == len(vw) and gout.shape[1] == len(vw) * D
    ops.emb_bwd_sgd(vw, vb, gout, lr, mode)
    ops.check_index_errors(sync=True)
    return [v.cpu().numpy() for v in vw]


def torch_sparse_step(op, rows, coll, tables, offs, idxs, dout, lr):
    """the reference's step per component: uncoalesced sparse COO gradients (indices verbatim, values = the gradient rows) consumed by
    torch.optim.SGD on the CPU"""
    D = tables[0][0].shape[1]
    out = []
    for t, ((W, Wr), n, c, off, idx) in enumerate(zip(tables, rows, coll, offs, idxs)):
        g = dout[:, t * D:(t + 1) * D]
        bag = H.bag_of(off, len(idx))
        if not c:
            comps = [(W, idx, g[bag])]
        else:
            _, sq, sr = H.np_qr_forward(W, Wr, idx, off, n, c, op)
            q, r, ok = H.qr_split(idx, n, c)
            assert ok.all()
            comps = [(W, q, (g * sr if op == "mult" else g)[bag]), (Wr, r, (g * sq if op == "mult" else g)[bag])]
        for Wc, ids, vals in comps:
            p = torch.nn.Parameter(torch.from_numpy(Wc.copy()))
            p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids).reshape(1, -1), torch.from_numpy(np.ascontiguousarray(vals)), size=Wc.shape)
            torch.optim.SGD([p], lr=lr).step()
            out.append((p.detach().numpy(), np.bincount(ids, minlength=Wc.shape[0])))
    return out


@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_deterministic_update_is_bit_exact_against_the_torch_sparse_step(op, idx_dtype):
    from dlrm_amd import ops
    case = update_case(11)
    got = device_step(ops.UPD_DETERMINISTIC, op, *case, 0.3, idx_dtype)
    want = torch_sparse_step(op, *case, 0.3)
    assert max(int(c.max()) for _, c in want) > 1000             # the remainder tables: thousands of duplicates per row
    for k, (g, (w, count)) in enumerate(zip(got, want)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "virtual table %d" % k


@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("mode_name", ["sorted", "atomic"])
def test_fast_updates_meet_their_contract_and_leave_other_rows_alone(op, mode_name):
    """SORTED / ATOMIC re-associate the sums of duplicate rows: the tolerance of tests/test_gpu_kernels.py (rtol 1e-5, atol 2e-5)"""
    from dlrm_amd import ops
    case = update_case(12)
    tables = case[2]
    got = device_step(ops.UPD_SORTED if mode_name == "sorted" else ops.UPD_ATOMIC, op, *case, 0.05)
    want = torch_sparse_step(op, *case, 0.05)
    start = []
    for w, r in tables:
        start += [w] if r is None else [w, r]
    for k, (g, (w, count), s) in enumerate(zip(got, want, start)):
        np.testing.assert_allclose(g, w, rtol=1e-5, atol=2e-5, err_msg="virtual table %d" % k)
        assert np.array_equal(g[count == 0], s[count == 0]), "virtual table %d: an untouched row changed" % k
    assert any((c == 0).any() for _, c in want)


# ------------------------------------------------------------------------------------------------ model against the live reference
def batch_to_dev(X, lS_o, lS_i, T, idx_dtype=torch.int64):
    return to_dev(X), [to_dev(o, idx_dtype) for o in lS_o], [to_dev(i, idx_dtype) for i in lS_i], to_dev(T)


def train_and_check(name, configure, make_opt=None, idx_dtype=torch.int64):
    from dlrm_amd import ops
    d, meta = load_golden("qr_training")
    case = meta["cases"][name]
    model = H.build_qr_model(case, meta["qr_threshold"], params=params_with_prefix(d, name + ".start"), seed=1).to(dev())
    configure(model)
    opt = (make_opt or (lambda ps: torch.optim.SGD(ps, lr=meta["lr"])))(model.parameters())
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
    final = params_with_prefix(d, name + ".final")
    sd = model.state_dict()
    assert list(sd) == list(final)
    for k, v in final.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v, rtol=1e-4, atol=2e-6, err_msg=k)
    return model, d, meta


@pytest.mark.parametrize("name", ["mult", "add", "onehot128"])
@pytest.mark.parametrize("mode_name", ["sorted", "atomic", "deterministic"])
def test_model_trains_like_the_live_reference(name, mode_name):
    from dlrm_amd import ops
    mode = {"sorted": ops.UPD_SORTED, "atomic": ops.UPD_ATOMIC, "deterministic": ops.UPD_DETERMINISTIC}[mode_name]
    train_and_check(name, lambda m: setattr(m, "emb_update_mode", mode))


@pytest.mark.parametrize("name", ["mult", "add", "onehot128"])
def test_model_trains_with_sparse_coo_gradients_and_torch_sgd(name):
    """fused_emb_update = False: weight_q.grad / weight_r.grad are the reference's sparse COO gradients, torch.optim.SGD consumes them"""
    def configure(m):
        m.fused_emb_update = False
    model, _, _ = train_and_check(name, configure, idx_dtype=torch.int32 if name == "add" else torch.int64)
    qr = [e for e in model.emb_l if hasattr(e, "weight_q")]
    assert qr and all(e.weight_q.grad is not None and e.weight_q.grad.is_sparse and e.weight_r.grad.is_sparse for e in qr)


def test_model_with_update_in_backward_and_overlap_falls_back_to_the_step_time_update():
    def configure(m):
        m.update_in_backward = True
    train_and_check("onehot128", configure)

    def configure2(m):
        m.overlap_streams = True
    train_and_check("mult", configure2)


def test_evaluate_inference_on_a_trained_qr_model():
    """evaluate.inference on the trained model: its metrics are dlrm_binary_metrics of the model's own predictions (the same kernels: the same
    bits), and those predictions are the torch CPU composition's from the trained parameters at the prediction tolerance"""
    from dlrm_amd import evaluate, ops
    model, d, meta = train_and_check("mult", lambda m: None)
    case = meta["cases"]["mult"]
    tm = H.TorchQRModel({k: v.cpu().numpy() for k, v in model.state_dict().items()}, case)
    batches, own, targets = [], [], []
    for X, lS_o, lS_i, T in H.case_batches(d, "mult", case, meta["steps"]):
        batches.append((torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i], torch.from_numpy(T)))
        with torch.no_grad():
            Z = model(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])
            np.testing.assert_allclose(Z.cpu().numpy(), tm.forward(X, lS_o, lS_i).numpy(), rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
        own.append(Z.reshape(-1))
        targets.append(T)
    got = evaluate.inference(model, batches, device=dev())
    want = ops.binary_metrics(torch.cat(own).contiguous(), to_dev(np.concatenate(targets).reshape(-1)))
    assert got["n"] == sum(len(t) for t in targets)
    assert got == want


def test_backward_twice_through_a_retained_graph():
    """the pooled sums stay with the autograd node: a second backward through a retained graph parks the same gradient again"""
    from dlrm_amd import ops
    d, meta = load_golden("qr_training")
    case = meta["cases"]["mult"]
    model = H.build_qr_model(case, meta["qr_threshold"], params=params_with_prefix(d, "mult.start"), seed=1).to(dev())
    X, lS_o, lS_i, T = batch_to_dev(*H.case_batches(d, "mult", case, 1)[0])
    E = model.loss_fn(model(X, lS_o, lS_i), T)
    E.backward(retain_graph=True)
    E.backward()
    assert len(model._pending_emb) == 2
    (_, _, g1, _), (_, _, g2, _) = model._pending_emb
    assert torch.equal(g1, g2)
    model._pending_emb.clear()
    ops.check_index_errors(sync=True)


def test_apply_emb_keeps_the_reference_shape():
    d, meta = load_golden("qr_training")
    case = meta["cases"]["add"]
    params = params_with_prefix(d, "add.start")
    model = H.build_qr_model(case, meta["qr_threshold"], params=params, seed=1).to(dev())
    X, lS_o, lS_i, _ = H.case_batches(d, "add", case, 1)[0]
    with torch.no_grad():
        ly = model.apply_emb([to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i], model.emb_l, model.v_W_l)
    assert len(ly) == len(case["ln_emb"]) and all(tuple(v.shape) == (X.shape[0], case["m_spa"]) for v in ly)
    for k, n in enumerate(case["ln_emb"]):
        if n > meta["qr_threshold"]:
            want = H.torch_qr_lookup(params[f"emb_l.{k}.weight_q"], params[f"emb_l.{k}.weight_r"], lS_i[k], lS_o[k], case["collisions"], "add")
        else:
            want = F.embedding_bag(torch.from_numpy(lS_i[k]), torch.from_numpy(params[f"emb_l.{k}.weight"]), torch.from_numpy(lS_o[k]), mode="sum").numpy()
        assert np.array_equal(ly[k].cpu().numpy(), want), k
    # the holder on its own: the same kernel for one table
    k = 2
    with torch.no_grad():
        one = model.emb_l[k](to_dev(lS_i[k]), to_dev(lS_o[k]))
    assert torch.equal(one, ly[k])
    one = model.emb_l[k](to_dev(lS_i[k]), to_dev(lS_o[k]))          # forward-only, also with gradients enabled: no autograd node
    assert torch.equal(one, ly[k]) and one.grad_fn is None and not one.requires_grad


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
@pytest.mark.parametrize("op", ["mult", "add"])
def test_launcher_with_qr_flag_matches_the_reference_cpu_run(op, tmp_path):
    """the UNMODIFIED reference CLI with --qr-flag: through dlrm_amd.launch on the GPU, and as it is on the CPU — every printed loss at 1e-5
    (identical seeds: identical numpy- and torch-drawn parameters, identical data)"""
    cli = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=31-32-1", "--arch-embedding-size=60-3-500-1200-250",
           "--data-generation=random", "--mini-batch-size=64", "--num-batches=8", "--nepochs=1", "--num-indices-per-lookup=1",
           "--num-indices-per-lookup-fixed=true", "--print-freq=1", "--print-time", "--numpy-rand-seed=71", "--learning-rate=0.01",
           "--loss-function=bce",            # losses near 0.7, printed with 6 decimals: the print's own 5e-7 is far below the 1e-5 relative bar
           "--qr-flag", "--qr-collisions=4", "--qr-threshold=200", "--qr-operation=" + op]
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


# ------------------------------------------------------------------------------------------------ refusals
def small_qr_model(**kw):
    d, meta = load_golden("qr_training")
    case = meta["cases"]["mult"]
    model = H.build_qr_model(case, meta["qr_threshold"], params=params_with_prefix(d, "mult.start"), seed=1, **kw).to(dev())
    return model, batch_to_dev(*H.case_batches(d, "mult", case, 1)[0])


def test_distributed_forward_refuses_qr_tables():
    model, (X, lS_o, lS_i, _) = small_qr_model()
    with pytest.raises(SystemExit, match="ERROR: QR embedding tables are single-process only"):
        model.distributed_forward(X, lS_o, lS_i)


def test_graphed_train_step_refuses_qr_tables():
    from dlrm_amd.graph import GraphedTrainStep
    model, _ = small_qr_model()
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for QR embedding tables"):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1))


def test_fused_rwsadagrad_refuses_qr_tables():
    from dlrm_amd.optim import FusedRWSAdagrad
    model, (X, lS_o, lS_i, T) = small_qr_model()
    opt = FusedRWSAdagrad(model.parameters(), lr=0.01)
    model.loss_fn(model(X, lS_o, lS_i), T).backward()
    with pytest.raises(SystemExit, match="ERROR: the fused row-wise Adagrad update is not built for QR embedding tables"):
        opt.step()


def test_quantize_embedding_refuses_a_qr_model_on_the_device():
    model, _ = small_qr_model()
    with pytest.raises(SystemExit, match="ERROR: 4 and 8-bit quantization with quotient remainder is not supported"):
        model.quantize_embedding(4)


def test_pooling_weights_handed_to_apply_emb_are_refused():
    model, (X, lS_o, lS_i, _) = small_qr_model()
    vws = [torch.ones(n, device=dev()) for n in [60, 3, 500, 1200, 250]]
    with pytest.raises(SystemExit, match="ERROR: quotient remainder with weighted pooling is not supported"):
        model.apply_emb(lS_o, lS_i, model.emb_l, vws)


# ------------------------------------------------------------------------------------------------ no regression
@pytest.mark.parametrize("fixture", ["config1_b128", "lr_schedule_onehot_d128"])
def test_a_model_without_qr_tables_gives_the_same_bits_with_and_without_the_flag(fixture):
    """qr_flag with a threshold above every table builds plain holders and takes the code a model without the flag takes: apply_emb and a
    deterministic-mode training step through sequential_forward give the same bits"""
    import dlrm_amd
    from dlrm_amd import ops
    d, meta = load_golden(fixture)
    T = len(meta["ln_emb"])
    results = []
    for flag in (False, True, False):
        np.random.seed(1)
        kw = dict(qr_flag=True, qr_collisions=4, qr_threshold=10 ** 9) if flag else {}
        model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]), "dot",
                                  sigmoid_top=meta["sigmoid_top"], loss_function="bce", **kw)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in params_with_prefix(d, "init").items()})
        model = model.to(dev())
        assert not model._has_qr(model.emb_l)
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
        results.append((ly, Z.detach().clone(), E.detach().clone(), {k: v.clone() for k, v in model.state_dict().items()}))
    for ly, Z, E, sd in results[1:]:
        assert torch.equal(ly, results[0][0]) and torch.equal(Z, results[0][1]) and torch.equal(E, results[0][2])
        assert list(sd) == list(results[0][3]) and all(torch.equal(sd[k], results[0][3][k]) for k in sd)
