"""The fused exact sparse Adagrad update on the device: dlrm_emb_bwd_adagrad through dlrm_amd.ops.emb_bwd_adagrad, dlrm_amd.optim.FusedAdagrad
and DLRM_Net.fused_adagrad.

Per touched row and per column the kernel computes, in fp32 (csrc/adagrad.hip, include/dlrm_hip.h):
    s = fadd(sum, fmul(g, g));   W = fma(-clr, g / (sqrt(s) + eps), W);   sum = s
where g is the row's coalesced gradient, summed by the walk the row-wise kernel uses.  Tolerances: W rtol 2e-4 / atol 2e-5 (the row-wise
kernel test's), sum rtol 2e-4 / atol 1e-6 against an fp64 restatement — torch.optim.Adagrad in fp32 stays within 0.02 / 0.18 of these bounds
against the same restatement, so a different fp32 summation order has room and a wrong formula does not."""
import numpy as np
import pytest
import torch

from conftest import golden_batches, load_golden, params_with_prefix

pytestmark = pytest.mark.gpu

W_TOL = dict(rtol=2e-4, atol=2e-5)
SUM_TOL = dict(rtol=2e-4, atol=1e-6)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def ragged(rng, B, rows, max_len, empty_frac=0.2):
    lens = rng.integers(0, max_len + 1, size=B)
    lens[rng.random(B) < empty_frac] = 0
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    idx = rng.integers(0, rows, size=int(lens.sum())).astype(np.int64)
    return off, idx


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


def bag_of(off, nnz):
    """bag of every lookup position"""
    lens = np.diff(np.concatenate([off, [nnz]]))
    return np.repeat(np.arange(off.shape[0]), lens)


def restate_fp64(W, S, idx, off, dV, psw, clr, eps):
    """the update in fp64, in place: np.add.at coalesce, then the three lines of the module docstring"""
    vals = dV[bag_of(off, idx.shape[0])].astype(np.float64)
    if psw is not None:
        vals = vals * psw.astype(np.float64)[:, None]
    G = np.zeros_like(W)
    np.add.at(G, idx, vals)
    r = np.unique(idx)
    g = G[r]
    s = S[r] + g * g
    W[r] = W[r] - clr * (g / (np.sqrt(s) + eps))
    S[r] = s


@pytest.mark.parametrize("D,rows,B,max_len", [(16, [3, 40, 5000], 300, 5), (128, [4, 10, 130, 100000], 700, 3),
                                              (6, [2, 9], 97, 4),            # scalar path
                                              (64, [1, 3], 5000, 2),         # runs of thousands crossing many groups: edge buffers + fix-up
                                              (200, [7, 300], 260, 6),
                                              (512, [5, 70], 130, 3),        # two column chunks per lane
                                              (128, [50] * 40, 64, 2)])      # more than 32 tables: two launch groups
@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_emb_bwd_adagrad_matches_an_fp64_restatement(D, rows, B, max_len, idx_dtype):
    """Two steps with accumulated state, ragged bags (10 % empty), per-sample weights on the last table.  initial_accumulator_value = 0.01:
    from a zero accumulator the first step is lr * sign(g), which turns the rounding noise of a near-zero g into a full-size difference."""
    from dlrm_amd import ops
    rng = np.random.default_rng(2000 + D + B)
    W32 = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    Ws = [w.astype(np.float64) for w in W32]
    Ss = [np.full((n, D), 0.01, dtype=np.float64) for n in rows]
    dW = [to_dev(w) for w in W32]
    dS = [torch.full((n, D), 0.01, dtype=torch.float32, device=dev()) for n in rows]
    for step in range(2):
        bags = [ragged(rng, B, n, max_len, empty_frac=0.1) for n in rows]
        psw = [None] * len(rows)
        psw[-1] = rng.standard_normal(bags[-1][1].shape[0]).astype(np.float32)
        dV = (rng.standard_normal((B, len(rows) * D)) * 0.1).astype(np.float32)
        clr, eps = 0.05 / (1 + step * 0.1), 1e-8
        for t, (W, S, (o, i), w) in enumerate(zip(Ws, Ss, bags, psw)):
            restate_fp64(W, S, i, o, dV[:, t * D:(t + 1) * D], w, float(np.float32(clr)), float(np.float32(eps)))
        bb = ops.BagBatch([to_dev(o, idx_dtype) for o, _ in bags], [to_dev(i, idx_dtype) for _, i in bags],
                          [None if w is None else to_dev(w) for w in psw])
        ops.emb_bwd_adagrad(dW, dS, bb, to_dev(dV), clr, eps)
        torch.cuda.synchronize()
        for t in range(len(rows)):
            got_s, got_w = dS[t].cpu().numpy(), dW[t].cpu().numpy()
            print("step %d table %d: max |dsum| %.3e  max |dW| %.3e" % (step, t, np.abs(got_s - Ss[t]).max(), np.abs(got_w - Ws[t]).max()))
            np.testing.assert_allclose(got_s, Ss[t], err_msg=f"sum {t} step {step}", **SUM_TOL)
            np.testing.assert_allclose(got_w, Ws[t], err_msg=f"W {t} step {step}", **W_TOL)


def test_unique_rows_give_torch_adagrads_accumulator_bits():
    """Every row is looked up at most once per step (ids from a permutation), no weights, 3 steps: `sum` is bit-equal to
    torch.optim.Adagrad's state["sum"] on the CPU from the same COO gradient (fmul + fadd is torch's state_sum.add_(grad.pow(2))); W is
    compared within the restatement test's tolerance."""
    from dlrm_amd import ops
    rng = np.random.default_rng(77)
    D, rows, B, L = 128, 5000, 300, 700
    lr, eps, acc0 = 0.05, 1e-10, 0.01
    W0 = rng.standard_normal((rows, D)).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(W0.copy()))
    opt = torch.optim.Adagrad([p], lr=lr, initial_accumulator_value=acc0, eps=eps)
    dW = [to_dev(W0)]
    dS = [torch.full((rows, D), acc0, dtype=torch.float32, device=dev())]
    for step in range(3):
        lens = rng.multinomial(L, np.full(B, 1.0 / B))                            # ragged, some bags empty, L lookups in all
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        idx = rng.permutation(rows)[:L].astype(np.int64)
        dV = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
        vals = dV[bag_of(off, L)]                                                 # the COO values: one gradient row per lookup
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(idx).reshape(1, -1), torch.from_numpy(vals), size=(rows, D))
        opt.step()
        ops.emb_bwd_adagrad(dW, dS, ops.BagBatch([to_dev(off)], [to_dev(idx)]), to_dev(dV), lr, eps)
        torch.cuda.synchronize()
        assert np.array_equal(dS[0].cpu().numpy(), opt.state[p]["sum"].numpy()), step
        np.testing.assert_allclose(dW[0].cpu().numpy(), p.detach().numpy(), err_msg=f"W step {step}", **W_TOL)


def test_one_column_equals_the_rowwise_kernel_bit_for_bit():
    """D = 1: the mean over one column is the column, so the [n, 1] accumulator and the row-wise [n] accumulator, and the tables, must
    come out bit-identical — the two apply steps share their expression forms."""
    from dlrm_amd import ops
    rng = np.random.default_rng(31)
    rows, B, max_len = [2, 300], 3000, 3
    W0 = [rng.standard_normal((n, 1)).astype(np.float32) for n in rows]
    We, Wr = [to_dev(w) for w in W0], [to_dev(w) for w in W0]
    Se = [torch.full((n, 1), 0.01, dtype=torch.float32, device=dev()) for n in rows]
    Sr = [torch.full((n,), 0.01, dtype=torch.float32, device=dev()) for n in rows]
    for step in range(2):
        bags = [ragged(rng, B, n, max_len) for n in rows]
        psw = [None, rng.standard_normal(bags[1][1].shape[0]).astype(np.float32)]
        dV = to_dev((rng.standard_normal((B, len(rows))) * 0.1).astype(np.float32))

        def bb():
            return ops.BagBatch([to_dev(o) for o, _ in bags], [to_dev(i) for _, i in bags], [None if w is None else to_dev(w) for w in psw])
        clr = 0.05 / (1 + step * 0.1)
        ops.emb_bwd_adagrad(We, Se, bb(), dV, clr, 1e-8)
        ops.emb_bwd_rowwise_adagrad(Wr, Sr, bb(), dV, clr, 1e-8)
        torch.cuda.synchronize()
        for t in range(len(rows)):
            assert np.array_equal(Se[t].cpu().numpy().reshape(-1), Sr[t].cpu().numpy()), (step, t)
            assert np.array_equal(We[t].cpu().numpy(), Wr[t].cpu().numpy()), (step, t)


def test_emb_bwd_adagrad_is_deterministic_and_touches_only_looked_up_rows():
    from dlrm_amd import ops
    rng = np.random.default_rng(5)
    D, rows, B = 32, [5, 2000], 4000
    bags = [ragged(rng, B, n, 3) for n in rows]
    dV = to_dev((rng.standard_normal((B, len(rows) * D)) * 0.1).astype(np.float32))
    W0 = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    S0 = [np.abs(rng.standard_normal((n, D))).astype(np.float32) for n in rows]
    bb = ops.BagBatch([to_dev(o) for o, _ in bags], [to_dev(i) for _, i in bags])
    results = []
    for _ in range(2):
        dW, dS = [to_dev(W) for W in W0], [to_dev(S) for S in S0]
        ops.emb_bwd_adagrad(dW, dS, bb, dV, 0.1, 1e-8)
        torch.cuda.synchronize()
        results.append(([w.cpu().numpy() for w in dW], [s.cpu().numpy() for s in dS]))
    for a, b in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert np.array_equal(a, b)                       # fixed summation order: bit-identical run to run
    touched = np.zeros(rows[1], dtype=bool)
    touched[bags[1][1]] = True
    assert (~touched).sum() > 0 and touched.sum() > 0
    assert np.array_equal(results[0][0][1][~touched].view(np.uint32), W0[1][~touched].view(np.uint32))
    assert np.array_equal(results[0][1][1][~touched].view(np.uint32), S0[1][~touched].view(np.uint32))
    assert not np.array_equal(results[0][1][1][touched], S0[1][touched])


def test_learning_rate_from_a_device_scalar_gives_the_by_value_bits():
    from dlrm_amd import ops
    rng = np.random.default_rng(17)
    D, rows, B = 32, [7, 3000, 90], 2500
    bags = [ragged(rng, B, n, 3) for n in rows]
    dV = to_dev((rng.standard_normal((B, len(rows) * D)) * 0.1).astype(np.float32))
    W0 = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    bb = ops.BagBatch([to_dev(o) for o, _ in bags], [to_dev(i) for _, i in bags])
    lr = 0.3125 + 1e-3                                           # not exactly representable: float(lr) is what both forms must use
    lr_t = torch.zeros(1, device=dev())
    ops.set_f32([lr_t], [lr])
    got = []
    for step in (lr, lr_t):
        dW = [to_dev(W) for W in W0]
        dS = [torch.full((n, D), 0.01, dtype=torch.float32, device=dev()) for n in rows]
        ops.emb_bwd_adagrad(dW, dS, bb, dV, step, 1e-8)
        torch.cuda.synchronize()
        got.append([w.cpu().numpy() for w in dW] + [s.cpu().numpy() for s in dS])
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_an_out_of_range_id_is_reported_and_skipped(idx_dtype):
    """the update equals the one with that lookup's gradient row zeroed (rtol 1e-5 / atol 1e-6, as the row-wise case in test_gpu_kernels.py)"""
    from dlrm_amd import ops
    rng = np.random.default_rng(3)
    D, rows, B = 16, [5, 300, 50], 64
    Ws = [rng.standard_normal((n, D)).astype(np.float32) for n in rows]
    idx = [rng.integers(0, n, size=B).astype(np.int64) for n in rows]
    bad = [i.copy() for i in idx]
    bad[0][3] = 5                      # == rows
    bad[1][17] = 1 << 20               # far beyond 2^row_bits
    bad[2][0] = -1 if idx_dtype == torch.int64 else 2 ** 31 - 1
    off = [np.arange(B)] * 3
    dout = rng.standard_normal((B, 3 * D)).astype(np.float32)
    dz = dout.copy()
    dz[3, 0:D] = 0; dz[17, D:2 * D] = 0; dz[0, 2 * D:3 * D] = 0

    def run(indices, g):
        Wd = [to_dev(w.copy()) for w in Ws]
        Sd = [torch.full((n, D), 0.01, dtype=torch.float32, device=dev()) for n in rows]
        bags = ops.BagBatch([to_dev(o).to(idx_dtype) for o in off], [to_dev(i).to(idx_dtype) for i in indices])
        ops.emb_bwd_adagrad(Wd, Sd, bags, to_dev(g), 0.1, 1e-10)
        torch.cuda.synchronize()
        return Wd + Sd

    ops.check_index_errors(sync=True)   # clean slate
    got = run(bad, dout)
    with pytest.raises(IndexError, match="out of range"):
        ops.check_index_errors(sync=True)
    ref = run(idx, dz)
    ops.check_index_errors(sync=True)
    for g, r in zip(got, ref):
        np.testing.assert_allclose(g.cpu().numpy(), r.cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_state_that_is_not_a_contiguous_fp32_rows_by_d_tensor_is_refused():
    """a wrong accumulator shape would be an out-of-bounds device write: refused on the host, nothing launched"""
    from dlrm_amd import ops
    rows, D, B = 40, 8, 16
    W = [torch.zeros(rows, D, device=dev())]
    bb = ops.BagBatch([torch.arange(B, device=dev())], [torch.zeros(B, dtype=torch.int64, device=dev())])
    dV = torch.zeros(B, D, device=dev())
    for bad in (torch.zeros(rows, device=dev()), torch.zeros(rows, D - 1, device=dev()), torch.zeros(rows - 1, D, device=dev()),
                torch.zeros(rows, D, dtype=torch.float64, device=dev()), torch.zeros(rows, 2 * D, device=dev())[:, ::2],
                torch.zeros(D, rows, device=dev()).t(), torch.zeros(rows, D)):
        with pytest.raises(RuntimeError):
            ops.emb_bwd_adagrad(W, [bad], bb, dV, 0.1, 1e-10)
    with pytest.raises(RuntimeError):
        ops.emb_bwd_adagrad(W, [], bb, dV, 0.1, 1e-10)


def build_model(meta, init, device):
    import dlrm_amd
    np.random.seed(0)
    m = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                          arch_interaction_op=meta.get("interaction", "dot"), arch_interaction_itself=meta["itself"], sigmoid_bot=-1,
                          sigmoid_top=meta["sigmoid_top"], loss_function=meta["loss"], loss_threshold=meta.get("loss_threshold", 0.0),
                          weighted_pooling=meta.get("weighted_pooling"))
    with torch.no_grad():
        sd = m.state_dict()
        assert set(sd.keys()) == set(init.keys())
        for k, v in init.items():
            sd[k].copy_(torch.from_numpy(v))
    return m.to(device)


@pytest.mark.parametrize("route", ["FusedAdagrad", "torch-adagrad-with-flag"])
def test_model_trains_like_torch_adagrad_on_the_cpu(route):
    """Three steps on the config1_b128 fixture against oracle.torch_port.TorchPortDLRM driven by torch.optim.Adagrad on the CPU, exactly as
    test_coo_escape_hatch_runs_any_torch_optimizer: loss 1e-5 relative, parameters rtol 2e-4 / atol 5e-6.  No table ever carries a .grad,
    and the tables' state["sum"] match the CPU optimizer's."""
    from dlrm_amd.optim import FusedAdagrad
    from oracle.torch_port import TorchPortDLRM
    d, meta = load_golden("config1_b128")
    device = dev()
    init = params_with_prefix(d, "init")
    model = build_model(meta, init, device)
    if route == "FusedAdagrad":
        opt = FusedAdagrad(model.parameters(), lr=0.05, initial_accumulator_value=0.1)
    else:
        model.fused_adagrad = True
        opt = torch.optim.Adagrad(model.parameters(), lr=0.05, initial_accumulator_value=0.1)
    ref = TorchPortDLRM({k: torch.from_numpy(v) for k, v in init.items()}, meta["sigmoid_top"], meta["itself"], meta["loss"], 0.05)
    ref.opt = torch.optim.Adagrad(list(ref.p.values()), lr=0.05, initial_accumulator_value=0.1)
    steps = 0
    for s, (X, lS_o, lS_i, T) in enumerate(golden_batches(d, meta)):
        Z = model(torch.from_numpy(X).to(device), [torch.from_numpy(o).to(device) for o in lS_o],
                  [torch.from_numpy(i).to(device) for i in lS_i])
        E = model.loss_fn(Z, torch.from_numpy(T).to(device))
        loss_ref, _ = ref.train_step(torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o],
                                     [torch.from_numpy(i) for i in lS_i], torch.from_numpy(T))
        assert abs(float(E.detach()) - loss_ref) <= 1e-5 * abs(loss_ref), (s, float(E.detach()), loss_ref)
        opt.zero_grad()
        E.backward()
        assert all(e.weight.grad is None for e in model.emb_l)
        opt.step()
        assert all(e.weight.grad is None for e in model.emb_l)
        steps += 1
    assert steps == meta["steps"] == 3
    sd = model.state_dict()
    for k, v in ref.p.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=2e-4, atol=5e-6, err_msg=k)
    for k, e in enumerate(model.emb_l):
        st = opt.state[e.weight]
        assert float(st["step"]) == steps
        np.testing.assert_allclose(st["sum"].cpu().numpy(), ref.opt.state[ref.p[f"emb_l.{k}.weight"]]["sum"].numpy(),
                                   err_msg=f"sum of table {k}", **SUM_TOL)
