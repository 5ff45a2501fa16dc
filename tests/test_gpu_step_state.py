"""Step state on the device (include/dlrm_hip.h "STEP STATE ON THE DEVICE", GraphedTrainStep(device_step_state=True)):

  * dlrm_philox_key_next draws, on the device, the key sequence the model draws on the host (dlrm_net._mix_seed; restated in
    tests/test_step_state_host.py key_sequence);
  * the *_devkey update calls leave the bits of the by-value calls given the same key (tables, and the row-wise Adagrad states);
  * a whole training step with bf16 tables (FusedSGD, FusedRWSAdagrad) or with FusedAdagrad, captured once and replayed under a learning
    rate that changes every step, is bit-identical to the same steps run eagerly — parameters, accumulators, losses — and the host
    mirrors (optimizer.state_dict() step counts, model._bf16_update_calls) read as if the replays had been eager steps: one more eager step
    on both models keeps them bit-identical; so does a re-capture after _drop_graph.

Shapes: T = 3 tables of (5, 64, 1000) rows (duplicates in every batch, runs that cross a 64-entry group of the sorted walk), B = 96,
D = 16 and 128 (4 and 32 lanes per row)."""
import numpy as np
import pytest
import torch

import test_step_state_host as S

pytestmark = pytest.mark.gpu

ROWS = (5, 64, 1000)
B = 96
NBATCH = 11


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def key_tensor(key):
    """the 64 bits of `key` as a 1-element int64 GPU tensor"""
    key &= 2 ** 64 - 1
    return torch.tensor([key - 2 ** 64 if key >= 2 ** 63 else key], dtype=torch.int64, device=dev())


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. the key sequence
@pytest.mark.parametrize("seed", S.SEEDS)
def test_philox_key_next_draws_the_hosts_key_sequence(seed):
    from dlrm_amd import ops
    from dlrm_amd.dlrm_net import _mix_seed
    state = ops.DeviceStepState(3, dev())
    keys = []
    for _ in range(6):
        ops.philox_key_next(seed, state.calls, state.key)
        keys += S.as_u64(state.key)
    assert keys == [_mix_seed(seed, n) for n in range(3, 9)] == S.key_sequence(seed, 3, 6)
    assert S.as_u64(state.calls) == [9]


def test_philox_key_next_refuses_what_is_not_two_distinct_int64_gpu_scalars():
    from dlrm_amd import ops
    a = torch.zeros(2, dtype=torch.int64, device=dev())
    with pytest.raises(RuntimeError, match="distinct tensors"):
        ops.philox_key_next(1, a[0:1], a[0:1])
    with pytest.raises(RuntimeError, match="1-element int64"):
        ops.philox_key_next(1, a, a[1:2])
    with pytest.raises(RuntimeError, match="must be torch.int64"):
        ops.philox_key_next(1, a[0:1].int(), a[1:2])
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.philox_key_next(1, a[0:1].cpu(), a[1:2])


# ------------------------------------------------------------------------------------------------ 2. the kernels
def kernel_case(D):
    """bags of 0..3 lookups; table 0 (5 rows): every row a run of ~30 lookups, crossing the walk's 64-entry groups"""
    rng = np.random.default_rng(700 + D)
    offs, idxs = [], []
    for n in ROWS:
        lens = rng.integers(0, 4, size=B)
        offs.append(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
        idxs.append(rng.integers(0, n, size=int(lens.sum()), dtype=np.int64))
    W = [torch.from_numpy(rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32)).to(torch.bfloat16) for n in ROWS]
    g = rng.uniform(-1.0, 1.0, size=(B, len(ROWS) * D)).astype(np.float32)
    state0 = [rng.uniform(0.0, 0.1, size=n).astype(np.float32) for n in ROWS]
    return W, offs, idxs, g, state0


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("D", [16, 128])
def test_device_key_updates_leave_the_bits_of_the_by_value_calls(D, rounding):
    from dlrm_amd import ops
    W, offs, idxs, g, state0 = kernel_case(D)
    assert max(np.bincount(idxs[0], minlength=ROWS[0])) > 20 and any(np.diff(np.append(o, i.size)).min() == 0 for o, i in zip(offs, idxs))
    key = 0xFEDCBA9876543210                     # (>= 2^63: both words of the key matter)
    gd = to_dev(g)

    def bags():
        return ops.BagBatch([to_dev(o) for o in offs], [to_dev(i) for i in idxs], None)

    def run(seed):
        sgd = [w.to(dev()) for w in W]
        ops.emb_bwd_sgd_bf16(sgd, bags(), gd, 0.25, rounding, seed)
        ada, st = [w.to(dev()) for w in W], [to_dev(s) for s in state0]
        ops.emb_bwd_rowwise_adagrad_bf16(ada, st, bags(), gd, 0.05, 1e-8, rounding, seed)
        ops.check_index_errors(sync=True)
        return sgd, ada, st

    by_value, on_device = run(key), run(key_tensor(key))
    for name, xs, ys in zip(("sgd tables", "adagrad tables", "adagrad states"), by_value, on_device):
        for t, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(bits(x), bits(y)), (name, t)
    assert any(not torch.equal(bits(x), bits(w.to(dev()))) for x, w in zip(by_value[0], W))          # (the update did something)
    if rounding == "stochastic":
        other = run(key_tensor(key ^ 1))
        assert any(not torch.equal(bits(x), bits(y)) for x, y in zip(other[0], on_device[0]))        # another key on the device: other bits


# ------------------------------------------------------------------------------------------------ 3. / 4. the whole step
CASES = {
    # name: (bf16 tables, optimizer, base lr)
    "bf16-sgd": (True, "FusedSGD", 0.5),
    "bf16-rwsadagrad": (True, "FusedRWSAdagrad", 0.05),
    "fp32-adagrad": (False, "FusedAdagrad", 0.05),
}
_batches = {}


def batches():
    """NBATCH batches, one lookup per bag (fixed shapes: what a replay takes), built once"""
    if not _batches:
        rng = np.random.default_rng(77)
        off = to_dev(np.arange(B, dtype=np.int64))
        for s in range(NBATCH):
            X = to_dev(rng.uniform(0.0, 1.0, size=(B, 13)).astype(np.float32))
            idx = [to_dev(rng.integers(0, n, size=B, dtype=np.int64)) for n in ROWS]
            T = to_dev(rng.integers(0, 2, size=(B, 1)).astype(np.float32))
            _batches[s] = (X, [off] * len(ROWS), idx, T)
    return _batches


def lr_at(base, s):
    return base * (1.0 + 0.25 * ((s * 5) % 7))           # another value at every step


def build(case, D):
    import dlrm_amd
    from dlrm_amd import optim
    bf16, opt_name, base = CASES[case]
    np.random.seed(3)
    torch.manual_seed(3)
    pairs = (1 + len(ROWS)) * len(ROWS) // 2
    model = dlrm_amd.DLRM_Net(D, np.asarray(ROWS), np.asarray([13, D]), np.asarray([D + pairs, 8, 1]), "dot", sigmoid_top=1).to(dev())
    if bf16:
        model.embedding_bfloat16("stochastic", 2 ** 63 + 2024)
    return model, getattr(optim, opt_name)(model.parameters(), lr=base), base


def eager_steps(model, opt, base, steps):
    losses = []
    for s in steps:
        for g in opt.param_groups:
            g["lr"] = lr_at(base, s)
        X, lS_o, lS_i, T = batches()[s]
        E = model.loss_fn(model(X, lS_o, lS_i), T)
        opt.zero_grad()
        E.backward()
        opt.step()
        losses.append(float(E.detach()))
        del E
    return losses


def graphed_steps(step, opt, base, steps):
    losses = []
    for s in steps:
        for g in opt.param_groups:
            g["lr"] = lr_at(base, s)
        losses.append(float(step(*batches()[s])))
    return losses


def assert_same_tree(a, b, where="state_dict"):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), where
        for k in a:
            assert_same_tree(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same_tree(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b)), where
    else:
        assert a == b, (where, a, b)


def assert_twins(eager, graphed):
    (me, oe), (mg, og) = eager, graphed
    torch.cuda.synchronize()
    sg = mg.state_dict()
    for k, v in me.state_dict().items():                   # tables and tower parameters
        assert v.dtype == sg[k].dtype and torch.equal(bits(v), bits(sg[k])), k
    assert_same_tree(oe.state_dict(), og.state_dict())     # accumulators, step counts, param groups (lr)
    assert getattr(me, "_bf16_update_calls", None) == getattr(mg, "_bf16_update_calls", None)


def twins(case, D):
    from dlrm_amd.graph import GraphedTrainStep
    me, oe, base = build(case, D)
    mg, og, _ = build(case, D)
    step = GraphedTrainStep(mg, og, warmup=2, device_step_state=True)
    me.overlap_streams, me.update_in_backward = mg.overlap_streams, mg.update_in_backward      # the schedule the constructor forced on mg
    return (me, oe), (mg, og), step, base


@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_graphed_steps_equal_eager_steps_and_the_host_mirrors_follow(case, D):
    eager, graphed, step, base = twins(case, D)
    le = eager_steps(*eager, base, range(7))
    lg = graphed_steps(step, graphed[1], base, range(7))               # 2 warm-up calls, the capture, 4 replays more
    assert le == lg, (le, lg)
    assert step.captures == 1 and step.lr_writes >= 4
    assert_twins(eager, graphed)
    steps = [st["step"] for st in graphed[1].state_dict()["state"].values()]
    assert all(int(n) == 7 for n in steps) and (len(steps) > 0) == (CASES[case][1] != "FusedSGD")       # (plain SGD keeps no step count)
    if CASES[case][0]:
        assert graphed[0]._bf16_update_calls == 7
    # one more EAGER step on both: the graphed model continues from settled counters
    assert eager_steps(*eager, base, [7]) == eager_steps(*graphed, base, [7])
    assert_twins(eager, graphed)
    assert step.captures == 1


@pytest.mark.parametrize("case", ["bf16-rwsadagrad", "fp32-adagrad"])
def test_a_recapture_continues_the_eager_sequence(case):
    D = 16
    eager, graphed, step, base = twins(case, D)
    le = eager_steps(*eager, base, range(10))
    lg = graphed_steps(step, graphed[1], base, range(5))               # warm-up, capture, 2 replays more
    step._drop_graph(batches()[0][0])
    if CASES[case][0]:
        assert graphed[0]._bf16_update_calls == 5                      # settled by _drop_graph
    lg += graphed_steps(step, graphed[1], base, range(5, 8))           # re-capture from the settled counter, 2 replays more
    assert step.captures == 2
    lg += eager_steps(*graphed, base, [8])                             # an eager step in between ...
    lg += graphed_steps(step, graphed[1], base, [9])                   # ... and a replay of the graph captured before it
    assert step.captures == 2
    assert le == lg, (le, lg)
    assert_twins(eager, graphed)
