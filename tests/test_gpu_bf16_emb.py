"""bfloat16 embedding tables on the device: dlrm_emb_fwd_bf16 / dlrm_emb_bwd_sgd_bf16 / dlrm_emb_bwd_rowwise_adagrad_bf16 through dlrm_amd.ops,
and DLRM_Net.embedding_bfloat16 forward / training / evaluation.

  * lookup: BIT-IDENTICAL to ops.emb_fwd on the same tables upcast to fp32 (bf16 -> fp32 is exact; same in-order fmaf chain);
  * updates, exact cases (one lookup per row, lr = 2^-3, |w| and |g| in [2^-4, 1]: w - lr*g is exact in fp64 and its fp32 rounding is the
    fma result): bit equality with the host restatement of tests/test_bf16_emb_host.py, nearest and stochastic;
  * row-wise Adagrad: oracle = ops.emb_bwd_rowwise_adagrad on the upcast tables; accumulators bit-identical, bf16 rows = the host rounding
    of that kernel's fp32 rows, exactly;
  * SGD with duplicates and pooling weights: inside the band rne(v - delta) .. rne(v + delta) of the fp64 value, delta the fp32 summation
    bound (L + 2) * 2^-24 * (|w| + lr * sum |psw * dout|); the band admits two values for at most 0.1 % of the elements;
  * model: a bf16 model against the fp32 model loaded with its tables upcast.
"""
import numpy as np
import pytest
import torch

import test_bf16_emb_host as H

pytestmark = pytest.mark.gpu


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


def random_bf16(rng, shape, lo=None):
    """bf16 bit patterns of values uniform in [-1, 1] (lo given: magnitudes in [lo, 1], random sign)"""
    if lo is None:
        x = rng.uniform(-1.0, 1.0, size=shape)
    else:
        x = rng.uniform(lo, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return H.round_nearest(x.astype(np.float32))


# ------------------------------------------------------------------------------------------------ lookup
ROWS = [1000, 50, 7]


@pytest.mark.parametrize("kind", ["onehot", "ragged"])
@pytest.mark.parametrize("D", [8, 16, 64, 128, 136, 256, 512, 12])       # 256 / 512: 32 / 64 lanes per bag; 12: the 2-bytes-per-lane path
def test_lookup_is_bit_identical_to_the_fp32_lookup_on_upcast_tables(D, kind):
    from dlrm_amd import ops
    rng = np.random.default_rng(1000 * D + len(kind))
    Tmax = 33
    tables = [bf16_table(random_bf16(rng, (ROWS[t % 3], D))) for t in range(Tmax)]
    up = [w.float() for w in tables]
    for B in (1, 37, 600):
        bags = [H.make_bags(rng, ROWS[t % 3], B, kind) for t in range(Tmax)]
        for T in (1, 3, 33):
            for idx_dtype in (torch.int64, torch.int32):
                for with_psw in (False, True):
                    lS_o = [to_dev(bags[t][0], idx_dtype) for t in range(T)]
                    lS_i = [to_dev(bags[t][1], idx_dtype) for t in range(T)]
                    psw = [to_dev(rng.uniform(0.5, 1.5, size=bags[t][1].size).astype(np.float32)) for t in range(T)] if with_psw else None
                    # into a wider feature buffer: out_ld > T*D, out offset by D (the bottom tower's slot)
                    feat_a = torch.full((B, (T + 2) * D), 7.0, dtype=torch.float32, device=dev())
                    feat_b = torch.full((B, (T + 2) * D), 7.0, dtype=torch.float32, device=dev())
                    ops.emb_fwd(up[:T], ops.BagBatch(lS_o, lS_i, psw), feat_a[:, D:(T + 1) * D])
                    ops.emb_fwd_bf16(tables[:T], ops.BagBatch(lS_o, lS_i, psw), feat_b[:, D:(T + 1) * D])
                    assert torch.equal(feat_a.view(torch.int32), feat_b.view(torch.int32)), (D, kind, B, T, idx_dtype, with_psw)
                    assert bool((feat_b[:, :D] == 7.0).all()) and bool((feat_b[:, (T + 1) * D:] == 7.0).all())
    ops.check_index_errors(sync=True)


def test_lookup_of_33_tables_crosses_the_launch_group_bit_identically():
    """33 tables of 7 rows, B = 5 bags of 0, 1, 5, 9 and 3 lookups: launch groups of 32 + 1; the first-row phase, one and two rounds of the
    4-deep loop and its tail"""
    from dlrm_amd import ops
    rng = np.random.default_rng(3333)
    T, rows, D, B = 33, 7, 16, 5
    tables = [bf16_table(random_bf16(rng, (rows, D))) for _ in range(T)]
    up = [w.float() for w in tables]
    off = np.asarray([0, 0, 1, 6, 15], dtype=np.int64)
    idx = [rng.integers(0, rows, size=18).astype(np.int64) for _ in range(T)]
    for idx_dtype in (torch.int64, torch.int32):
        for with_psw in (False, True):
            lS_o = [to_dev(off, idx_dtype)] * T
            lS_i = [to_dev(i, idx_dtype) for i in idx]
            psw = [to_dev(rng.uniform(0.5, 1.5, size=18).astype(np.float32)) for _ in range(T)] if with_psw else None
            # into a wider feature buffer, as the test above
            a = torch.full((B, (T + 2) * D), 7.0, dtype=torch.float32, device=dev())
            b = torch.full((B, (T + 2) * D), 7.0, dtype=torch.float32, device=dev())
            ops.emb_fwd(up, ops.BagBatch(lS_o, lS_i, psw), a[:, D:(T + 1) * D])
            ops.emb_fwd_bf16(tables, ops.BagBatch(lS_o, lS_i, psw), b[:, D:(T + 1) * D])
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (idx_dtype, with_psw)
            assert bool((b[:, :D] == 7.0).all()) and bool((b[:, (T + 1) * D:] == 7.0).all())
    ops.check_index_errors(sync=True)


@pytest.mark.parametrize("D", [16, 12])
def test_lookup_skips_and_reports_out_of_range_ids(D):
    from dlrm_amd import ops
    rng = np.random.default_rng(5)
    B, rows = 37, 50
    w = bf16_table(random_bf16(rng, (rows, D)))
    off, idx = H.make_bags(rng, rows, B, "ragged")
    bad = idx.copy()
    bad[3], bad[11], bad[20] = rows, -1, 10 ** 9
    good = np.ones(idx.size, dtype=bool)
    good[[3, 11, 20]] = False
    out_bad = torch.empty((B, D), dtype=torch.float32, device=dev())
    ops.check_index_errors(sync=True)
    ops.emb_fwd_bf16([w], ops.BagBatch([to_dev(off)], [to_dev(bad)]), out_bad)
    with pytest.raises(IndexError, match="embedding index out of range: table 0"):
        ops.check_index_errors(sync=True)
    # the same bags without the skipped lookups
    keep_off = np.array([int(good[:o].sum()) for o in off], dtype=np.int64)
    out_ref = torch.empty((B, D), dtype=torch.float32, device=dev())
    ops.emb_fwd([w.float()], ops.BagBatch([to_dev(keep_off)], [to_dev(idx[good])]), out_ref)
    ops.check_index_errors(sync=True)
    assert torch.equal(out_bad.view(torch.int32), out_ref.view(torch.int32))


def test_operands_other_than_contiguous_bf16_gpu_tables_raise():
    from dlrm_amd import ops
    off, idx = to_dev(np.arange(4, dtype=np.int64)), to_dev(np.zeros(4, dtype=np.int64))
    out = torch.empty((4, 8), dtype=torch.float32, device=dev())
    w = torch.zeros((5, 8), dtype=torch.bfloat16, device=dev())
    with pytest.raises(RuntimeError, match="must be torch.bfloat16"):
        ops.emb_fwd_bf16([w.float()], ops.BagBatch([off], [idx]), out)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.emb_fwd_bf16([w.cpu()], ops.BagBatch([off], [idx]), out)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.emb_fwd_bf16([torch.zeros((5, 16), dtype=torch.bfloat16, device=dev())[:, ::2]], ops.BagBatch([off], [idx]), out)
    with pytest.raises(RuntimeError, match="'nearest' or 'stochastic'"):
        ops.emb_bwd_sgd_bf16([w], ops.BagBatch([off], [idx]), out, 0.1, rounding="up")


# ------------------------------------------------------------------------------------------------ updates, exact cases
LR = 2.0 ** -3


def exact_case(rng, T, rows, B, D):
    """one lookup per row (distinct rows per table), |w| and |g| in [2^-4, 1]"""
    W = [random_bf16(rng, (rows, D), lo=2.0 ** -4) for _ in range(T)]
    idx = [rng.permutation(rows)[:B].astype(np.int64) for _ in range(T)]
    g = (rng.uniform(2.0 ** -4, 1.0, size=(B, T * D)) * rng.choice([-1.0, 1.0], size=(B, T * D))).astype(np.float32)
    return W, idx, g


def exact_expected(W, idx, g, D, mode, seed, table0=0):
    out = []
    for t, (w, ix) in enumerate(zip(W, idx)):
        v = (H.bf16_to_f32(w[ix]).astype(np.float64) - LR * g[:, t * D:(t + 1) * D].astype(np.float64)).astype(np.float32)   # exact, then ONE fp32 rounding
        e = w.copy()
        e[ix] = H.round_rows(v, mode, table0 + t, ix, seed)
        out.append(e)
    return out


def run_sgd(W, idx, g, mode, seed, table0=0, psw=None, offs=None, lr=LR):
    from dlrm_amd import ops
    B = g.shape[0]
    tabs = [bf16_table(w) for w in W]
    lS_o = [to_dev(np.arange(B, dtype=np.int64) if offs is None else offs[t]) for t in range(len(W))]
    bags = ops.BagBatch(lS_o, [to_dev(i) for i in idx], None if psw is None else [to_dev(p) for p in psw])
    ops.emb_bwd_sgd_bf16(tabs, bags, to_dev(g), lr, mode, seed, table0)
    ops.check_index_errors(sync=True)
    return [bits_of(t) for t in tabs]


@pytest.mark.parametrize("D", [16, 128, 6])          # 6: the one-column-per-lane path
def test_sgd_exact_cases_equal_the_host_restatement_bit_for_bit(D):
    rng = np.random.default_rng(D)
    W, idx, g = exact_case(rng, 3, 1000, 600, D)
    near = run_sgd(W, idx, g, "nearest", 0)
    for got, want in zip(near, exact_expected(W, idx, g, D, "nearest", 0)):
        assert np.array_equal(got, want)
    s1, s2 = 0x0123456789ABCDEF, 77
    a = run_sgd(W, idx, g, "stochastic", s1)
    for got, want in zip(a, exact_expected(W, idx, g, D, "stochastic", s1)):
        assert np.array_equal(got, want)
    b = run_sgd(W, idx, g, "stochastic", s2)
    for got, want in zip(b, exact_expected(W, idx, g, D, "stochastic", s2)):
        assert np.array_equal(got, want)
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))             # two seeds: different bits
    again = run_sgd(W, idx, g, "stochastic", s1)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))             # the same seed twice: the same bits


def test_sgd_launch_grouping_does_not_change_the_random_stream():
    D, T, rows, B = 16, 33, 100, 64
    rng = np.random.default_rng(33)
    W, idx, g = exact_case(rng, T, rows, B, D)
    seed = 4242
    want = exact_expected(W, idx, g, D, "stochastic", seed)
    whole = run_sgd(W, idx, g, "stochastic", seed)                          # 33 tables: launch groups of 32 + 1 inside the call
    for got, w in zip(whole, want):
        assert np.array_equal(got, w)
    tail = run_sgd(W[32:], idx[32:], np.ascontiguousarray(g[:, 32 * D:]), "stochastic", seed, table0=32)      # the caller cuts the list itself
    assert np.array_equal(tail[0], want[32])
    head = run_sgd(W[:5], idx[:5], np.ascontiguousarray(g[:, :5 * D]), "stochastic", seed, table0=0)
    assert all(np.array_equal(x, y) for x, y in zip(head, want[:5]))


# ------------------------------------------------------------------------------------------------ duplicates: Adagrad and SGD
def dup_case(seed, D, with_psw):
    """three tables in one launch, B = 600: [0] 1000 rows, ragged bags (duplicates inside one 64-entry group) with row 5 named by 200 more
    lookups (a run that crosses group boundaries); [1] 4000 rows, ragged (mostly one or two lookups per touched row); [2] 3 rows, one lookup
    per bag (every run goes through pass 2).  The few hot rows carry wide fp32 summation bounds (L ~ 200 lookups per row of the 3-row
    table: the SGD band admits two bf16 values for about a tenth of their elements); the many cold rows keep the share of such elements
    over the whole launch under the 0.1 % cap — a property of these inputs alone, computed on the host."""
    rng = np.random.default_rng(seed)
    B, rows = 600, [1000, 4000, 3]
    W = [random_bf16(rng, (n, D)) for n in rows]
    offs, idxs = [], []
    for t, n in enumerate(rows):
        off, idx = H.make_bags(rng, n, B, "onehot" if t == 2 else "ragged")
        if t == 0:
            idx[rng.permutation(idx.size)[:200]] = 5
        offs.append(off)
        idxs.append(idx)
    g = rng.uniform(-1.0, 1.0, size=(B, 3 * D)).astype(np.float32)
    psw = [rng.uniform(0.5, 1.5, size=i.size).astype(np.float32) for i in idxs] if with_psw else None
    return W, offs, idxs, g, psw


@pytest.mark.parametrize("with_psw", [False, True])
@pytest.mark.parametrize("D", [16, 128, 6, 66, 512])          # 66 / 512: two chunks per lane at one / four columns per lane
def test_rowwise_adagrad_has_the_fp32_kernels_accumulators_and_its_rows_rounded_once(D, with_psw):
    from dlrm_amd import ops
    W, offs, idxs, g, psw = dup_case(100 + D, D, with_psw)
    assert int((idxs[0] == 5).sum()) >= 130
    rng = np.random.default_rng(D)
    state0 = [rng.uniform(0.0, 0.1, size=w.shape[0]).astype(np.float32) for w in W]
    lr, eps = 0.01, 1e-8

    def bags():
        return ops.BagBatch([to_dev(o) for o in offs], [to_dev(i) for i in idxs], None if psw is None else [to_dev(p) for p in psw])

    ref_w = [bf16_table(w).float() for w in W]
    ref_s = [to_dev(s) for s in state0]
    ops.emb_bwd_rowwise_adagrad(ref_w, ref_s, bags(), to_dev(g), lr, eps)
    ref_rows = [w.cpu().numpy() for w in ref_w]
    for mode, seed in (("nearest", 0), ("stochastic", 31337)):
        tabs = [bf16_table(w) for w in W]
        st = [to_dev(s) for s in state0]
        ops.emb_bwd_rowwise_adagrad_bf16(tabs, st, bags(), to_dev(g), lr, eps, mode, seed)
        ops.check_index_errors(sync=True)
        for t in range(3):
            assert torch.equal(st[t].view(torch.int32), ref_s[t].view(torch.int32)), (mode, t)
            touched = np.unique(idxs[t])
            want = W[t].copy()
            want[touched] = H.round_rows(ref_rows[t][touched], mode, t, touched, seed)
            assert np.array_equal(bits_of(tabs[t]), want), (mode, t)


def test_rowwise_adagrad_of_a_row_with_700_lookups_has_the_fp32_kernels_accumulator():
    """one row named by 700 of 760 lookups: its run spans more than nine 64-entry groups, so the fix-up pass's 8-deep loop and its tail both
    run; accumulators and rows as in the test above"""
    from dlrm_amd import ops
    rng = np.random.default_rng(700)
    D, rows, B = 16, 50, 760
    W = random_bf16(rng, (rows, D))
    idx = rng.integers(0, rows, size=B).astype(np.int64)
    idx[rng.permutation(B)[:700]] = 5
    g = rng.uniform(-1.0, 1.0, size=(B, D)).astype(np.float32)
    state0 = rng.uniform(0.0, 0.1, size=rows).astype(np.float32)
    lr, eps = 0.01, 1e-8

    def bags():
        return ops.BagBatch([to_dev(np.arange(B, dtype=np.int64))], [to_dev(idx)])

    ref_w, ref_s = [bf16_table(W).float()], [to_dev(state0)]
    ops.emb_bwd_rowwise_adagrad(ref_w, ref_s, bags(), to_dev(g), lr, eps)
    ref_rows = ref_w[0].cpu().numpy()
    touched = np.unique(idx)
    for mode, seed in (("nearest", 0), ("stochastic", 31337)):
        tabs, st = [bf16_table(W)], [to_dev(state0)]
        ops.emb_bwd_rowwise_adagrad_bf16(tabs, st, bags(), to_dev(g), lr, eps, mode, seed)
        ops.check_index_errors(sync=True)
        assert torch.equal(st[0].view(torch.int32), ref_s[0].view(torch.int32)), mode
        want = W.copy()
        want[touched] = H.round_rows(ref_rows[touched], mode, 0, touched, seed)
        assert np.array_equal(bits_of(tabs[0]), want), mode


def sgd_band(W, offs, idxs, g, psw, D, lr):
    """per table: (touched rows, rne(v - delta), rne(v + delta)) as fp32 values of the bf16 results"""
    out = []
    B = g.shape[0]
    for t, (w, off, idx) in enumerate(zip(W, offs, idxs)):
        bag = np.searchsorted(off, np.arange(idx.size), side="right") - 1
        p = np.ones(idx.size) if psw is None else psw[t].astype(np.float64)
        contrib = p[:, None] * g[bag, t * D:(t + 1) * D].astype(np.float64)
        rows = w.shape[0]
        s = np.zeros((rows, D)); sa = np.zeros((rows, D)); L = np.zeros(rows)
        np.add.at(s, idx, contrib); np.add.at(sa, idx, np.abs(contrib)); np.add.at(L, idx, 1)
        touched = np.unique(idx)
        w64 = H.bf16_to_f32(w[touched]).astype(np.float64)
        v = w64 - lr * s[touched]
        delta = (L[touched, None] + 2) * 2.0 ** -24 * (np.abs(w64) + lr * sa[touched])
        lo = H.bf16_to_f32(H.round_nearest((v - delta).astype(np.float32)))
        hi = H.bf16_to_f32(H.round_nearest((v + delta).astype(np.float32)))
        out.append((touched, np.minimum(lo, hi), np.maximum(lo, hi)))
    assert B == off.size
    return out


@pytest.mark.parametrize("with_psw", [False, True])
@pytest.mark.parametrize("D", [16, 128, 6])
def test_sgd_with_duplicates_lies_in_the_band_of_the_fp64_value(D, with_psw):
    W, offs, idxs, g, psw = dup_case(200 + D, D, with_psw)
    got = run_sgd(W, idxs, g, "nearest", 0, psw=psw, offs=offs, lr=LR)
    band = sgd_band(W, offs, idxs, g, psw, D, LR)
    two, total = 0, 0
    for t, (touched, lo, hi) in enumerate(band):
        val = H.bf16_to_f32(got[t][touched])
        assert bool(((val >= lo) & (val <= hi)).all()), t
        untouched = np.setdiff1d(np.arange(W[t].shape[0]), touched)
        assert np.array_equal(got[t][untouched], W[t][untouched])
        two += int((lo != hi).sum())
        total += lo.size
    print("band admits two values for %d of %d elements (%.4f %%)" % (two, total, 100.0 * two / total))
    assert two <= 0.001 * total


# ------------------------------------------------------------------------------------------------ model
MODEL_ROWS = [1000, 50, 7]


def build_pair(D=16, rounding="nearest", seed=0):
    """B: a bf16 model; A: the fp32 model loaded with B's tables upcast"""
    import dlrm_amd
    models = []
    for _ in range(2):
        np.random.seed(3)
        torch.manual_seed(3)
        pairs = (1 + len(MODEL_ROWS)) * len(MODEL_ROWS) // 2
        models.append(dlrm_amd.DLRM_Net(D, np.asarray(MODEL_ROWS), np.asarray([13, D]), np.asarray([D + pairs, 8, 1]), "dot", sigmoid_top=1).to(dev()))
    a, b = models
    b.embedding_bfloat16(rounding, seed)
    a.load_state_dict({k: v.float() for k, v in b.state_dict().items()})
    return a, b


def batch(kind, B=128, seed=9):
    rng = np.random.default_rng(seed)
    X = to_dev(rng.uniform(0.0, 1.0, size=(B, 13)).astype(np.float32))
    bags = [H.make_bags(rng, n, B, kind) for n in MODEL_ROWS]
    target = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
    return X, [to_dev(o) for o, _ in bags], [to_dev(i) for _, i in bags], target, [i for _, i in bags]


def one_step(model, opt, X, lS_o, lS_i, target):
    opt.zero_grad()
    loss = model.loss_fn(model(X, lS_o, lS_i), target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return float(loss.detach())


def check_rows_against_fp32(a, b, before, idxs, exact_everywhere):
    for t, (ea, eb) in enumerate(zip(a.emb_l, b.emb_l)):
        A = ea.weight.detach().cpu().numpy()
        got = bits_of(eb.weight)
        counts = np.bincount(idxs[t], minlength=MODEL_ROWS[t])
        single, multi, none = np.where(counts == 1)[0], np.where(counts > 1)[0], np.where(counts == 0)[0]
        assert np.array_equal(got[none], before[t][none])                                   # untouched rows are unchanged
        assert np.array_equal(got[single], H.round_nearest(A[single]))                      # one lookup: the nearest rounding of A's row, exactly
        if exact_everywhere:
            assert np.array_equal(got[multi], H.round_nearest(A[multi]))
        val, ref = H.bf16_to_f32(got[multi]), A[multi]
        mag = np.maximum(np.maximum(np.abs(val), np.abs(ref)), np.float32(2.0 ** -126))
        ulp = 2.0 ** (np.floor(np.log2(mag)) - 7)
        assert bool((np.abs(val.astype(np.float64) - ref.astype(np.float64)) <= ulp).all())          # within one bf16 ulp of A's row
        assert (single.size > 0 and none.size > 0) if MODEL_ROWS[t] >= 1000 else multi.size > 0          # (the batch exercises every class of row)


def test_model_forward_is_bit_equal_and_one_sgd_step_follows_the_fp32_model():
    from dlrm_amd.optim import FusedSGD
    a, b = build_pair()
    X, lS_o, lS_i, target, idxs = batch("ragged")
    with torch.no_grad():
        za, zb = a(X, lS_o, lS_i), b(X, lS_o, lS_i)
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32))
    before = [bits_of(e.weight) for e in b.emb_l]
    la = one_step(a, FusedSGD(a.parameters(), lr=0.5), X, lS_o, lS_i, target)
    lb = one_step(b, FusedSGD(b.parameters(), lr=0.5), X, lS_o, lS_i, target)
    assert la == lb
    assert all(e.weight.dtype == torch.bfloat16 for e in b.emb_l)
    check_rows_against_fp32(a, b, before, idxs, exact_everywhere=False)
    for pa, pb in zip(a.bot_l.parameters(), b.bot_l.parameters()):
        assert torch.equal(pa, pb)


def test_model_rowwise_adagrad_state_is_bit_equal_to_the_fp32_models():
    from dlrm_amd.optim import FusedRWSAdagrad
    a, b = build_pair()
    X, lS_o, lS_i, target, idxs = batch("ragged")
    before = [bits_of(e.weight) for e in b.emb_l]
    oa, ob = FusedRWSAdagrad(a.parameters(), lr=0.05), FusedRWSAdagrad(b.parameters(), lr=0.05)
    assert one_step(a, oa, X, lS_o, lS_i, target) == one_step(b, ob, X, lS_o, lS_i, target)
    for ea, eb in zip(a.emb_l, b.emb_l):
        sa, sb = oa.state[ea.weight]["momentum"], ob.state[eb.weight]["momentum"]
        assert sb.dtype == torch.float32 and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    check_rows_against_fp32(a, b, before, idxs, exact_everywhere=True)


def test_three_stochastic_steps_with_a_fixed_seed_are_reproducible():
    from dlrm_amd.optim import FusedSGD
    runs = []
    for _ in range(2):
        _, b = build_pair(rounding="stochastic", seed=2024)
        opt = FusedSGD(b.parameters(), lr=0.5)
        losses = [one_step(b, opt, *batch("ragged", seed=20 + s)[:4]) for s in range(3)]
        runs.append((losses, [bits_of(e.weight) for e in b.emb_l]))
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))
    _, c = build_pair(rounding="stochastic", seed=2025)                       # another seed: other bits
    optc = FusedSGD(c.parameters(), lr=0.5)
    for s in range(3):
        one_step(c, optc, *batch("ragged", seed=20 + s)[:4])
    assert any(not np.array_equal(x, bits_of(e.weight)) for x, e in zip(runs[0][1], c.emb_l))


def test_fixed_pooling_weights_overlap_streams_and_inference_run_on_the_bf16_model():
    import dlrm_amd
    from dlrm_amd import evaluate
    from dlrm_amd.optim import FusedSGD
    np.random.seed(3)
    torch.manual_seed(3)
    pairs = (1 + len(MODEL_ROWS)) * len(MODEL_ROWS) // 2
    m = dlrm_amd.DLRM_Net(16, np.asarray(MODEL_ROWS), np.asarray([13, 16]), np.asarray([16 + pairs, 8, 1]), "dot", sigmoid_top=1,
                          weighted_pooling="fixed").to(dev())
    m.embedding_bfloat16("stochastic", 1)
    m.overlap_streams = True
    X, lS_o, lS_i, target, idxs = batch("ragged")
    before = [bits_of(e.weight) for e in m.emb_l]
    opt = FusedSGD(m.parameters(), lr=0.5)
    for _ in range(2):                          # (the second step launches the update from backward, on the side stream)
        assert np.isfinite(one_step(m, opt, X, lS_o, lS_i, target))
    m._join_side_stream()
    torch.cuda.synchronize()
    assert any(not np.array_equal(x, bits_of(e.weight)) for x, e in zip(before, m.emb_l))
    res = evaluate.inference(m, [(X, lS_o, lS_i, target)])
    assert 0.0 <= res["round_accuracy"] <= 1.0 if "round_accuracy" in res else len(res) > 0


def test_one_hot_d128_takes_the_two_kernel_form_and_matches_the_fused_fp32_forward():
    from dlrm_amd import ops
    a, b = build_pair(D=128)
    X, lS_o, lS_i, _, _ = batch("onehot")
    saved = ops.timers
    try:
        with torch.no_grad():
            ops.timers = ops.KernelTimers()
            za = a(X, lS_o, lS_i)
            cats_a = set(ops.timers.summary())
            ops.timers = ops.KernelTimers()
            zb = b(X, lS_o, lS_i)
            cats_b = set(ops.timers.summary())
    finally:
        ops.timers = saved
    assert "emb_interact_fwd" in cats_a and "emb_fwd" not in cats_a               # the fp32 model took the fused lookup + interaction kernels
    assert "emb_fwd_bf16" in cats_b and "interact_fwd" in cats_b and "emb_interact_fwd" not in cats_b
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32))
