"""Quotient-remainder (QR) embedding tables, host side: the restatements the GPU tests rely on, pinned against torch on the CPU, and
the model's construction pinned against the live reference's (tests/golden/qr_training.npz, written by tools/make_golden_qr.py).

  * index split: q = (id / c).long() is a FLOAT32 division in the reference; the numpy restatement equals torch's on ids around and above
    2^24, where it differs from id // c — and for n = 40,000,000, c = 4 two ids get the quotient 10,000,000 = rows_q, which is no row;
  * forward and the two sparse gradients: a numpy restatement (in-order fp32 sums, then one multiply / add) equals autograd through
    F.embedding_bag composed as tricks/qr_embedding_bag.py composes it;
  * DLRM_Net(qr_flag=True) built on the CPU from the fixture's seeds has the fixture's state_dict keys, shapes and bits;
  * the fixture's step-0 predictions are reproduced by the torch-operator composition from its stored parameters.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, params_with_prefix

PRED_RTOL, PRED_ATOL = 2e-5, 1e-6        # the project's prediction tolerance (tests/test_gpu_model.py)


# ------------------------------------------------------------------------------------------------ restatements
def rows_q(n: int, c: int) -> int:
    return -(-int(n) // int(c))


def float_quotient(ids: np.ndarray, c: int) -> np.ndarray:
    """(input / c).long() of the reference: both operands to float32 (round to nearest), IEEE division, truncation"""
    return (np.asarray(ids).astype(np.float32) / np.float32(c)).astype(np.int64)


def qr_split(ids: np.ndarray, n: int, c: int):
    """(q, r, ok): ok is False for an id outside [0, n) or whose quotient is >= ceil(n / c) — the lookups the kernels skip"""
    ids = np.asarray(ids, dtype=np.int64)
    q = float_quotient(ids, c)
    r = np.remainder(ids, c)
    ok = (ids >= 0) & (ids < n) & (q >= 0) & (q < rows_q(n, c))
    return q, r, ok


def torch_split(ids: np.ndarray, c: int):
    t = torch.from_numpy(np.asarray(ids))
    return (t / c).long().numpy(), torch.remainder(t, c).long().numpy()


def bag_of(off: np.ndarray, nnz: int) -> np.ndarray:
    ends = np.concatenate([np.asarray(off[1:], dtype=np.int64), [nnz]])
    return np.repeat(np.arange(len(off)), ends - np.asarray(off, dtype=np.int64))


def np_qr_forward(Wq, Wr, ids, off, n, c, op):
    """(out, sq, sr): per component the in-order fp32 sum over the bag from +0.0, then ONE fp32 multiply / add; skipped lookups add nothing"""
    q, r, ok = qr_split(ids, n, c)
    B, D = len(off), Wq.shape[1]
    sq, sr = np.zeros((B, D), dtype=np.float32), np.zeros((B, D), dtype=np.float32)
    bag = bag_of(off, len(ids))
    for i in range(len(ids)):                                   # index order: np.add.at would also do, a loop states the order
        if ok[i]:
            sq[bag[i]] += Wq[q[i]]
            sr[bag[i]] += Wr[r[i]]
    return (sq * sr if op == "mult" else sq + sr), sq, sr


def np_qr_grads(Wq, Wr, ids, off, n, c, op, dout):
    """dense images of the two sparse gradients: every lookup i of bag b adds dout[b] o' sr[b] to row q_i of weight_q and dout[b] o' sq[b] to
    row r_i of weight_r ("add": both dout[b]); float64 accumulation (the order of a coalesced sparse gradient is torch's business)"""
    _, sq, sr = np_qr_forward(Wq, Wr, ids, off, n, c, op)
    q, r, ok = qr_split(ids, n, c)
    bag = bag_of(off, len(ids))
    gq_row = dout * sr if op == "mult" else dout
    gr_row = dout * sq if op == "mult" else dout
    gq, gr = np.zeros(Wq.shape), np.zeros(Wr.shape)
    np.add.at(gq, q[ok], gq_row[bag[ok]].astype(np.float64))
    np.add.at(gr, r[ok], gr_row[bag[ok]].astype(np.float64))
    return gq, gr


def torch_qr_bag(Wq: torch.Tensor, Wr: torch.Tensor, ids: torch.Tensor, off: torch.Tensor, c: int, op: str, sparse=True):
    """the reference's composition (tricks/qr_embedding_bag.py forward, mode="sum") from torch's operators"""
    eq = F.embedding_bag((ids / c).long(), Wq, off, mode="sum", sparse=sparse)
    er = F.embedding_bag(torch.remainder(ids, c).long(), Wr, off, mode="sum", sparse=sparse)
    return eq * er if op == "mult" else eq + er


def torch_qr_lookup(Wq, Wr, ids, off, c, op) -> np.ndarray:
    with torch.no_grad():
        return torch_qr_bag(torch.from_numpy(Wq), torch.from_numpy(Wr), torch.from_numpy(np.asarray(ids, dtype=np.int64)),
                            torch.from_numpy(np.asarray(off, dtype=np.int64)), c, op).numpy()


def make_bags(rng, n: int, B: int, kind: str):
    if kind == "onehot":
        return np.arange(B, dtype=np.int64), rng.integers(0, n, size=B).astype(np.int64)
    if kind == "empty":
        return np.zeros(B, dtype=np.int64), np.zeros(0, dtype=np.int64)
    lens = rng.integers(0, {"ragged": 39, "short": 4}[kind] + 1, size=B)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), rng.integers(0, n, size=int(lens.sum())).astype(np.int64)


class TorchQRModel:
    """The reference's forward / SGD training of a DLRM with QR tables from torch's CPU operators and autograd (dlrm_s_pytorch.py:407-462,
    483-510, 587-612, 1611-1621), from a state_dict given as numpy arrays.  Tables with `emb_l.{k}.weight_q` are QR tables."""

    def __init__(self, params: dict, case: dict):
        self.p = {k: torch.from_numpy(np.array(v, dtype=np.float32)).requires_grad_(True) for k, v in params.items()}
        self.case = case

    def tower(self, x, prefix, sig):
        i = 0
        while f"{prefix}.{2 * i}.weight" in self.p:
            x = F.linear(x, self.p[f"{prefix}.{2 * i}.weight"], self.p[f"{prefix}.{2 * i}.bias"])
            x = torch.sigmoid(x) if i == sig else torch.relu(x)
            i += 1
        return x

    def forward(self, X, lS_o, lS_i):
        c, op = self.case["collisions"], self.case["op"]
        x = self.tower(torch.from_numpy(np.asarray(X, dtype=np.float32)), "bot_l", -1)
        ly = []
        for k in range(len(lS_i)):
            ids, off = torch.from_numpy(np.asarray(lS_i[k], dtype=np.int64)), torch.from_numpy(np.asarray(lS_o[k], dtype=np.int64))
            if f"emb_l.{k}.weight_q" in self.p:
                ly.append(torch_qr_bag(self.p[f"emb_l.{k}.weight_q"], self.p[f"emb_l.{k}.weight_r"], ids, off, c, op))
            else:
                ly.append(F.embedding_bag(ids, self.p[f"emb_l.{k}.weight"], off, mode="sum", sparse=True))
        B, d = x.shape
        T = torch.cat([x] + ly, dim=1).view((B, -1, d))
        Z = torch.bmm(T, torch.transpose(T, 1, 2))
        ni = T.shape[1]
        li = torch.tensor([i for i in range(ni) for j in range(i)])
        lj = torch.tensor([j for i in range(ni) for j in range(i)])
        return self.tower(torch.cat([x, Z[:, li, lj]], dim=1), "top_l", self.case["sigmoid_top"])

    def train_step(self, opt, X, lS_o, lS_i, T):
        Z = self.forward(X, lS_o, lS_i)
        E = F.binary_cross_entropy(Z, torch.from_numpy(np.asarray(T, dtype=np.float32)))
        opt.zero_grad()
        E.backward()
        opt.step()
        return float(E.item()), Z.detach().numpy()

    def state(self):
        return {k: v.detach().numpy().copy() for k, v in self.p.items()}


def case_batches(d: dict, name: str, case: dict, steps: int):
    T = len(case["ln_emb"])
    return [(d[f"{name}.s{s}.X"], [d[f"{name}.s{s}.off{k}"] for k in range(T)], [d[f"{name}.s{s}.idx{k}"] for k in range(T)], d[f"{name}.s{s}.T"])
            for s in range(steps)]


def build_qr_model(case: dict, threshold: int, params=None, seed=None, **kw):
    import dlrm_amd
    if seed is not None:
        np.random.seed(seed)
        torch.manual_seed(seed)
    model = dlrm_amd.DLRM_Net(case["m_spa"], np.asarray(case["ln_emb"]), np.asarray(case["ln_bot"]), np.asarray(case["ln_top"]), "dot",
                              sigmoid_top=case["sigmoid_top"], loss_function="bce", qr_flag=True, qr_operation=case["op"],
                              qr_collisions=case["collisions"], qr_threshold=threshold, **kw)
    if params is not None:
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return model


# ------------------------------------------------------------------------------------------------ index split
@pytest.mark.parametrize("c", [2, 3, 4, 7, 60, 1000])
def test_float_quotient_equals_torch_and_integer_division_below_2_pow_24(c):
    rng = np.random.default_rng(c)
    ids = np.concatenate([np.arange(0, 5000), rng.integers(0, 2 ** 24, size=200000), np.arange(2 ** 24 - 5000, 2 ** 24)]).astype(np.int64)
    tq, tr = torch_split(ids, c)
    assert np.array_equal(float_quotient(ids, c), tq)
    assert np.array_equal(tq, ids // c)
    assert np.array_equal(np.remainder(ids, c), tr)


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("c", [2, 3, 4, 7, 60, 1000])
def test_float_quotient_equals_torch_above_2_pow_24(c, dtype):
    rng = np.random.default_rng(100 + c)
    ids = np.concatenate([np.arange(2 ** 24 - 3000, 2 ** 24 + 3000), rng.integers(2 ** 24, 2 ** 31 - 1, size=300000),
                          np.arange(39_884_406 - 3000, 39_884_406), np.arange(2 ** 31 - 3000, 2 ** 31 - 1)]).astype(dtype)
    tq, tr = torch_split(ids, c)
    assert np.array_equal(float_quotient(ids, c), tq)
    assert np.array_equal(np.remainder(ids.astype(np.int64), c), tr)


def test_float_quotient_differs_from_integer_division_on_a_criteo_sized_table():
    n, c = 39_884_406, 4
    ids = np.arange(n - 3_000_000, n, dtype=np.int64)
    tq, _ = torch_split(ids, c)
    q, r, ok = qr_split(ids, n, c)
    assert np.array_equal(q, tq) and ok.all()
    assert int((q != ids // c).sum()) == 1_125_000


def test_the_two_ids_of_a_40m_table_whose_quotient_is_no_row():
    n, c = 40_000_000, 4
    ids = np.arange(n - 5_000_000, n, dtype=np.int64)               # the top eighth
    tq, _ = torch_split(ids, c)
    q, r, ok = qr_split(ids, n, c)
    assert np.array_equal(q, tq)
    assert rows_q(n, c) == 10_000_000
    assert ids[~ok].tolist() == [39_999_998, 39_999_999] and q[~ok].tolist() == [10_000_000, 10_000_000]
    with pytest.raises((IndexError, RuntimeError)):                  # torch rejects them
        F.embedding_bag(torch.from_numpy(tq[-2:]), torch.zeros((16, 2)).expand(rows_q(n, c), 2), torch.tensor([0]), mode="sum")
    out_of_range = np.array([-1, n, n + 7], dtype=np.int64)
    assert not qr_split(out_of_range, n, c)[2].any()


# ------------------------------------------------------------------------------------------------ forward and gradients
@pytest.mark.parametrize("op", ["mult", "add"])
@pytest.mark.parametrize("kind", ["ragged", "short", "empty", "onehot"])
@pytest.mark.parametrize("n,c,D", [(1000, 4, 16), (250, 7, 12), (501, 60, 8)])
def test_numpy_restatement_equals_autograd_through_embedding_bag(op, kind, n, c, D):
    rng = np.random.default_rng(n + c + D)
    B = 97
    Wq = rng.uniform(0.1, 1.0, size=(rows_q(n, c), D)).astype(np.float32)
    Wr = rng.uniform(0.1, 1.0, size=(c, D)).astype(np.float32)
    off, ids = make_bags(rng, n, B, kind)
    dout = rng.standard_normal((B, D)).astype(np.float32)
    tWq, tWr = torch.from_numpy(Wq).requires_grad_(True), torch.from_numpy(Wr).requires_grad_(True)
    out = torch_qr_bag(tWq, tWr, torch.from_numpy(ids), torch.from_numpy(off), c, op)
    out.backward(torch.from_numpy(dout))
    got, sq, sr = np_qr_forward(Wq, Wr, ids, off, n, c, op)
    assert np.array_equal(got, out.detach().numpy())                 # in-order sums + one operation: the same bits
    if kind == "empty":
        assert (got == 0).all()
    assert tWq.grad.is_sparse and tWr.grad.is_sparse
    gq, gr = np_qr_grads(Wq, Wr, ids, off, n, c, op, dout)
    # a row of the remainder table sums up to B * 39 / c terms: fp32 accumulation in torch's coalesce, float64 here
    terms = max(len(ids), 1)
    for mine, theirs in ((gq, tWq.grad.to_dense().numpy()), (gr, tWr.grad.to_dense().numpy())):
        scale = np.abs(mine).max() + 1e-30
        assert np.abs(mine - theirs).max() <= terms * 2.0 ** -23 * max(scale, 1.0) * 4


# ------------------------------------------------------------------------------------------------ the model and the fixture
@pytest.mark.parametrize("name", ["mult", "add", "onehot128"])
def test_model_built_on_the_cpu_has_the_fixture_state_dict_bit_for_bit(name):
    d, meta = load_golden("qr_training")
    case = meta["cases"][name]
    model = build_qr_model(case, meta["qr_threshold"], seed=case["seed"])
    want = params_with_prefix(d, name + ".init")
    sd = model.state_dict()
    assert list(sd) == list(want)
    n_qr = 0
    for k, n in enumerate(case["ln_emb"]):
        if n > meta["qr_threshold"]:
            n_qr += 1
            assert tuple(sd[f"emb_l.{k}.weight_q"].shape) == (rows_q(n, case["collisions"]), case["m_spa"])
            assert tuple(sd[f"emb_l.{k}.weight_r"].shape) == (case["collisions"], case["m_spa"])
            assert float(sd[f"emb_l.{k}.weight_q"].min()) >= np.float32(np.sqrt(1 / n))          # U(sqrt(1/n), 1): the reference's quirk
        else:
            assert tuple(sd[f"emb_l.{k}.weight"].shape) == (n, case["m_spa"])
    assert n_qr >= 1
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy().view(np.uint32), v.view(np.uint32)), k


@pytest.mark.parametrize("name", ["mult", "add", "onehot128"])
def test_fixture_is_reproduced_by_the_torch_operator_composition(name):
    d, meta = load_golden("qr_training")
    case = meta["cases"][name]
    start = params_with_prefix(d, name + ".start")
    init = params_with_prefix(d, name + ".init")
    for k in start:                                                  # start = init with the QR tables scaled (tools/make_golden_qr.py)
        s = np.float32(case["qr_scale"]) if k.endswith(("weight_q", "weight_r")) else np.float32(1)
        assert np.array_equal(start[k], init[k] * s), k
    tm = TorchQRModel(start, case)
    opt = torch.optim.SGD(list(tm.p.values()), lr=meta["lr"])
    for s, (X, lS_o, lS_i, T) in enumerate(case_batches(d, name, case, meta["steps"])):
        loss, pred = tm.train_step(opt, X, lS_o, lS_i, T)
        np.testing.assert_allclose(pred, d[f"{name}.s{s}.pred"], rtol=PRED_RTOL, atol=PRED_ATOL, err_msg="step %d" % s)
        assert abs(loss - float(d[f"{name}.s{s}.loss"])) <= 1e-5 * abs(float(d[f"{name}.s{s}.loss"]))
    final = params_with_prefix(d, name + ".final")
    for k, v in tm.state().items():
        np.testing.assert_allclose(v, final[k], rtol=1e-4, atol=2e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def _tiny_case(op="mult", collisions=4):
    ln_emb = [300, 3, 40]
    return {"m_spa": 8, "ln_emb": ln_emb, "ln_bot": [13, 8], "ln_top": [8 + 6, 1], "sigmoid_top": 0, "op": op, "collisions": collisions}


def test_concat_is_refused_with_its_reason():
    with pytest.raises(SystemExit, match=r"ERROR: --qr-operation=concat makes a QR table 2\*D wide"):
        build_qr_model(_tiny_case(op="concat"), 200)


def test_weighted_pooling_with_qr_is_refused_in_the_reference_wording():
    with pytest.raises(SystemExit, match="ERROR: quotient remainder with weighted pooling is not supported"):
        build_qr_model(_tiny_case(), 200, weighted_pooling="fixed")


def test_quantize_embedding_on_a_qr_model_is_refused_in_the_reference_wording():
    model = build_qr_model(_tiny_case(), 200)
    with pytest.raises(SystemExit, match="ERROR: 4 and 8-bit quantization with quotient remainder is not supported"):
        model.quantize_embedding(8)


def test_bad_collisions_and_operation_are_refused():
    with pytest.raises(SystemExit, match="ERROR: --qr-collisions must be at least 1"):
        build_qr_model(_tiny_case(collisions=0), 200)
    with pytest.raises(SystemExit, match="ERROR: --qr-operation=max is not supported"):
        build_qr_model(_tiny_case(op="max"), 200)


def test_mixed_dimension_refusal_is_unchanged():
    import dlrm_amd
    with pytest.raises(SystemExit, match="ERROR: mixed-dimension embeddings are not supported by the MI355X DLRM_Net"):
        dlrm_amd.DLRM_Net(8, np.asarray([300, 3]), np.asarray([13, 8]), np.asarray([11, 1]), "dot", md_flag=True, md_threshold=200)


def test_torchrec_variants_refuse_qr_tables():
    """their constructors take no qr_* argument, so the public interface cannot ask for a QR table; the refusal guards create_emb, which
    ShardedDLRM calls itself and a subclass may reach with the qr_* attributes set — reached here the same way"""
    import inspect
    from dlrm_amd import torchrec_variant as tv
    for cls in (tv.DLRM, tv.ShardedDLRM, tv.DLRM_DCN):
        assert not any(p.startswith("qr_") or p == "kwargs" for p in inspect.signature(cls.__init__).parameters), cls.__name__
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.qr_flag, m.qr_threshold, m.qr_collisions, m.qr_operation = True, 200, 4, "mult"
        with pytest.raises(SystemExit, match="ERROR: QR embeddings are built for DLRM_Net only"):
            m.create_emb(8, np.asarray([300]))


def test_a_model_below_the_threshold_is_the_plain_model():
    """qr_flag with no table above the threshold: plain holders, numpy-drawn, the bits of a model built without the flag"""
    import dlrm_amd
    case = _tiny_case()
    np.random.seed(5)
    a = dlrm_amd.DLRM_Net(8, np.asarray(case["ln_emb"]), np.asarray(case["ln_bot"]), np.asarray(case["ln_top"]), "dot")
    b = build_qr_model(case, 1000, seed=5)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not b._has_qr(b.emb_l)
