"""Mixed-dimension (MD) embedding tables, host side: the restatements the GPU tests rely on, pinned against torch on the CPU, and the
model's construction pinned against the live reference's (tests/golden/md_training.npz, written by tools/make_golden_md.py).

  * the restated md_solver equals the dimensions the reference's solver gave for the fixture, and hand-checked values for the 26
    Criteo-Terabyte tables at alpha 0, 0.3 and 1, rounded to powers of two and not;
  * DLRM_Net(md_flag=True) built on the CPU from the fixture's seeds has the fixture's state_dict keys, shapes and bits;
  * the fixture's losses, predictions and final parameters are reproduced by the torch-operator composition (F.embedding_bag + F.linear,
    autograd) from its stored parameters: that composition is the oracle of tests/test_gpu_md_emb.py;
  * every refusal that needs no GPU, and the plain [n, base] table of an md_flag model at or below the threshold.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, params_with_prefix

PRED_RTOL, PRED_ATOL = 2e-5, 1e-6        # the project's prediction tolerance (tests/test_gpu_model.py)

CRITEO_TB_ROWS = [39884406, 39043, 17289, 7420, 20263, 3, 7120, 1543, 63, 38532951, 2953546, 403346, 10, 2208, 11938, 155,
                  4, 976, 14, 39979771, 25641295, 39664984, 585935, 12972, 108, 36]
# d0 = 128.  Checked by hand: 128 * (3 / n)^alpha, never below 1, rounded half to even; then 2^round(log2 d).  alpha = 0.3: n = 4 gives
# 128 * 0.75^0.3 = 117.4, n = 10 gives 128 * 0.3^0.3 = 89.2 -> 64, the 40 M-row tables 0.93 -> 1.  alpha = 1: 384 / n (n = 10: 38.4 -> 32, n = 63: 6.1 -> 8).
TB_DIMS = {
    (0.0, True): [128] * 26,
    (0.0, False): [128] * 26,
    (0.3, True): [1, 8, 8, 16, 8, 128, 16, 16, 64, 1, 2, 4, 64, 16, 8, 32, 128, 32, 64, 1, 1, 1, 4, 8, 32, 64],
    (0.3, False): [1, 7, 10, 12, 9, 128, 12, 20, 51, 1, 2, 4, 89, 18, 11, 39, 117, 23, 81, 1, 1, 1, 3, 10, 44, 61],
    (1.0, True): [1, 1, 1, 1, 1, 128, 1, 1, 8, 1, 1, 1, 32, 1, 1, 2, 128, 1, 32, 1, 1, 1, 1, 1, 4, 8],
    (1.0, False): [1, 1, 1, 1, 1, 128, 1, 1, 6, 1, 1, 1, 38, 1, 1, 2, 96, 1, 27, 1, 1, 1, 1, 1, 4, 11],
}
CASES = ["pow2", "odd", "onehot128"]


# ------------------------------------------------------------------------------------------------ restatements
class TorchMDModel:
    """The reference's forward / SGD training of a DLRM with mixed-dimension tables from torch's CPU operators and autograd
    (tricks/md_embedding_bag.py PrEmbeddingBag.forward; dlrm_s_pytorch.py:407-462, 483-510, 587-612, 1611-1621), from a state_dict given as
    numpy arrays.  Tables with `emb_l.{k}.embs.weight` are MD tables; one with `emb_l.{k}.proj.weight` is projected."""

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
        x = self.tower(torch.from_numpy(np.asarray(X, dtype=np.float32)), "bot_l", -1)
        ly = []
        for k in range(len(lS_i)):
            ids, off = torch.from_numpy(np.asarray(lS_i[k], dtype=np.int64)), torch.from_numpy(np.asarray(lS_o[k], dtype=np.int64))
            if f"emb_l.{k}.embs.weight" in self.p:
                e = F.embedding_bag(ids, self.p[f"emb_l.{k}.embs.weight"], off, mode="sum", sparse=True)
                if f"emb_l.{k}.proj.weight" in self.p:
                    e = F.linear(e, self.p[f"emb_l.{k}.proj.weight"])
                ly.append(e)
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


def make_bags(rng, n: int, B: int, kind: str):
    if kind == "onehot":
        return np.arange(B, dtype=np.int64), rng.integers(0, n, size=B).astype(np.int64)
    if kind == "empty":
        return np.zeros(B, dtype=np.int64), np.zeros(0, dtype=np.int64)
    lens = rng.integers(0, {"ragged": 39, "short": 4}[kind] + 1, size=B)
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), rng.integers(0, n, size=int(lens.sum())).astype(np.int64)


def bag_of(off: np.ndarray, nnz: int) -> np.ndarray:
    ends = np.concatenate([np.asarray(off[1:], dtype=np.int64), [nnz]])
    return np.repeat(np.arange(len(off)), ends - np.asarray(off, dtype=np.int64))


def torch_pooled(W: np.ndarray, ids, off) -> np.ndarray:
    """torch's CPU F.embedding_bag(mode="sum"): the in-order fp32 sum per column"""
    with torch.no_grad():
        return F.embedding_bag(torch.from_numpy(np.asarray(ids, dtype=np.int64)), torch.from_numpy(W), torch.from_numpy(np.asarray(off, dtype=np.int64)),
                               mode="sum").numpy()


def case_batches(d: dict, name: str, case: dict, steps: int):
    T = len(case["ln_emb"])
    return [(d[f"{name}.s{s}.X"], [d[f"{name}.s{s}.off{k}"] for k in range(T)], [d[f"{name}.s{s}.idx{k}"] for k in range(T)], d[f"{name}.s{s}.T"])
            for s in range(steps)]


def build_md_model(case: dict, threshold: int, params=None, seed=None, dims=None, **kw):
    import dlrm_amd
    if seed is not None:
        np.random.seed(seed)
        torch.manual_seed(seed)
    model = dlrm_amd.DLRM_Net(list(case["dims"]) if dims is None else dims, np.asarray(case["ln_emb"]), np.asarray(case["ln_bot"]),
                              np.asarray(case["ln_top"]), "dot", sigmoid_top=case["sigmoid_top"], loss_function="bce", md_flag=True,
                              md_threshold=threshold, **kw)
    if params is not None:
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return model


# ------------------------------------------------------------------------------------------------ md_solver
def test_md_solver_gives_the_dimensions_the_reference_solver_gave_for_the_fixture():
    from dlrm_amd import ops
    d, meta = load_golden("md_training")
    case = meta["cases"]["pow2"]
    got = ops.md_solver(torch.tensor(case["ln_emb"]), case["alpha"], d0=case["d0"], round_dim=case["round_dims"])
    assert got.dtype == torch.int64
    assert got.tolist() == d["pow2.dims"].tolist() == case["dims"] == [8, 16, 4, 4, 4]


@pytest.mark.parametrize("alpha,rounded", sorted(TB_DIMS))
def test_md_solver_on_the_criteo_terabyte_tables(alpha, rounded):
    from dlrm_amd import ops
    got = ops.md_solver(CRITEO_TB_ROWS, alpha, d0=128, round_dim=rounded).tolist()
    assert got == TB_DIMS[(alpha, rounded)]
    n = np.asarray(CRITEO_TB_ROWS, dtype=np.float64)                 # the rule itself, in float64
    want = np.rint(np.maximum(128 * (n.min() / n) ** alpha, 1))
    if rounded:
        want = 2 ** np.rint(np.log2(want))
    assert got == want.astype(np.int64).tolist()
    assert got[CRITEO_TB_ROWS.index(3)] == 128                       # the smallest table keeps d0


def test_md_solver_pieces():
    from dlrm_amd import ops
    assert ops.pow_2_round(torch.tensor([1, 3, 5, 6, 11, 12, 23, 89, 117])).tolist() == [1, 4, 4, 8, 8, 16, 32, 64, 128]
    assert ops.alpha_power_rule(torch.tensor([10., 100., 1000.]), 0.5, d0=16).tolist() == [16, 5, 2]
    with pytest.raises(ValueError):
        ops.alpha_power_rule(torch.tensor([10.]), 0.5)
    lay = ops.MDLayout([8, 16, 4, 3, 4, 16, 1])
    assert [(d, ks) for d, ks, _ in lay.groups] == [(16, [1, 5]), (8, [0]), (4, [2, 4]), (3, [3]), (1, [6])]
    assert all(c0 % 4 == 0 for _, _, c0 in lay.groups) and lay.width % 4 == 0
    assert lay.cols == [32, 0, 40, 48, 44, 16, 52] and lay.width == 56


# ------------------------------------------------------------------------------------------------ the model and the fixture
@pytest.mark.parametrize("name", CASES)
def test_model_built_on_the_cpu_has_the_fixture_state_dict_bit_for_bit(name):
    d, meta = load_golden("md_training")
    case = meta["cases"][name]
    model = build_md_model(case, meta["md_threshold"], seed=case["seed"])
    want = params_with_prefix(d, name + ".init")
    sd = model.state_dict()
    assert list(sd) == list(want)
    base = max(case["dims"])
    n_proj = 0
    for k, (n, dk) in enumerate(zip(case["ln_emb"], case["dims"])):
        assert tuple(sd[f"emb_l.{k}.embs.weight"].shape) == (n, dk)
        if dk < base:
            n_proj += 1
            assert tuple(sd[f"emb_l.{k}.proj.weight"].shape) == (base, dk)
        else:
            assert f"emb_l.{k}.proj.weight" not in sd                 # nn.Identity
    assert n_proj >= 2
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy().view(np.uint32), v.view(np.uint32)), k
    assert model._has_md(model.emb_l)


@pytest.mark.parametrize("name", CASES)
def test_fixture_is_reproduced_by_the_torch_operator_composition(name):
    d, meta = load_golden("md_training")
    case = meta["cases"][name]
    tm = TorchMDModel(params_with_prefix(d, name + ".init"), case)
    opt = torch.optim.SGD(list(tm.p.values()), lr=meta["lr"])
    for s, (X, lS_o, lS_i, T) in enumerate(case_batches(d, name, case, meta["steps"])):
        loss, pred = tm.train_step(opt, X, lS_o, lS_i, T)
        np.testing.assert_allclose(pred, d[f"{name}.s{s}.pred"], rtol=PRED_RTOL, atol=PRED_ATOL, err_msg="step %d" % s)
        assert abs(loss - float(d[f"{name}.s{s}.loss"])) <= 1e-5 * abs(float(d[f"{name}.s{s}.loss"]))
    final = params_with_prefix(d, name + ".final")
    moved = 0
    for k, v in tm.state().items():
        np.testing.assert_allclose(v, final[k], rtol=1e-4, atol=2e-6, err_msg=k)
        moved += int(k.endswith("proj.weight") and not np.array_equal(v, d[f"{name}.init.{k}"]))
    assert moved >= 2                                                # the projections are trained


def test_a_table_at_or_below_the_threshold_is_a_plain_table_of_the_base_width():
    case = {"ln_emb": [300, 3, 40, 200], "ln_bot": [13, 8], "ln_top": [8 + 10, 1], "sigmoid_top": 0}
    model = build_md_model(case, 200, dims=[2, 8, 4, 4], seed=3)
    sd = model.state_dict()
    assert tuple(sd["emb_l.0.embs.weight"].shape) == (300, 2) and tuple(sd["emb_l.0.proj.weight"].shape) == (8, 2)
    for k, n in ((1, 3), (2, 40), (3, 200)):                          # (n == threshold is not above it)
        assert tuple(sd[f"emb_l.{k}.weight"].shape) == (n, 8)
        assert float(sd[f"emb_l.{k}.weight"].abs().max()) <= np.float32(np.sqrt(1 / n))
        assert f"emb_l.{k}.embs.weight" not in sd
    assert model._emb_dim(model.emb_l) == 8
    # dimensions as a numpy array or a tensor (md_solver's result) build the same model
    for dims in (np.asarray([2, 8, 4, 4]), torch.tensor([2, 8, 4, 4]), [2.0, 8.0, 4.0, 4.0]):
        other = build_md_model(case, 200, dims=dims, seed=3).state_dict()
        assert list(other) == list(sd) and all(torch.equal(other[k], sd[k]) for k in sd)


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def _tiny_case():
    return {"ln_emb": [300, 3, 40], "dims": [2, 8, 4], "ln_bot": [13, 8], "ln_top": [8 + 6, 1], "sigmoid_top": 0}


def test_weighted_pooling_with_md_is_refused_in_the_reference_wording():
    with pytest.raises(SystemExit, match="ERROR: mixed dimensions with weighted pooling is not supported"):
        build_md_model(_tiny_case(), 2, weighted_pooling="fixed")


def test_quantize_embedding_on_an_md_model_is_refused_in_the_reference_wording():
    model = build_md_model(_tiny_case(), 2)
    with pytest.raises(SystemExit, match="ERROR: 4 and 8-bit quantization with mixed dimensions is not supported"):
        model.quantize_embedding(8)


def test_md_with_qr_is_refused():
    with pytest.raises(SystemExit, match="ERROR: --md-flag and --qr-flag cannot be combined"):
        build_md_model(_tiny_case(), 2, qr_flag=True, qr_collisions=4, qr_threshold=2)


def test_bottom_tower_width_other_than_the_base_dimension_is_refused():
    case = dict(_tiny_case(), ln_bot=[13, 4])
    with pytest.raises(SystemExit, match="ERROR: arch-sparse-feature-size 8 does not match last dim of bottom mlp 4"):
        build_md_model(case, 2)


def test_wrong_number_of_dimensions_is_refused():
    with pytest.raises(SystemExit, match="ERROR: --md-flag needs one embedding dimension >= 1 per table"):
        build_md_model(_tiny_case(), 2, dims=[8, 8])
    with pytest.raises(SystemExit, match="ERROR: --md-flag needs one embedding dimension >= 1 per table"):
        build_md_model(_tiny_case(), 2, dims=[8, 0, 4])


def test_scalar_dimension_keeps_the_old_refusal():
    import dlrm_amd
    with pytest.raises(SystemExit, match="ERROR: mixed-dimension embeddings are not supported by the MI355X DLRM_Net"):
        dlrm_amd.DLRM_Net(8, np.asarray([300, 3]), np.asarray([13, 8]), np.asarray([11, 1]), "dot", md_flag=True, md_threshold=200)


def test_distributed_forward_refuses_md_tables():
    model = build_md_model(_tiny_case(), 2)
    with pytest.raises(SystemExit, match="ERROR: mixed-dimension embedding tables are single-process only"):
        model.distributed_forward(torch.zeros((2, 13)), [torch.zeros(2, dtype=torch.int64)] * 3, [torch.zeros(2, dtype=torch.int64)] * 3)


def test_graphed_train_step_refuses_md_tables():
    from dlrm_amd.graph import GraphedTrainStep
    model = build_md_model(_tiny_case(), 2)
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for mixed-dimension embedding tables"):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1))


def test_rowwise_adagrad_refuses_md_tables():
    from dlrm_amd.optim import FusedRWSAdagrad
    model = build_md_model(_tiny_case(), 2)
    opt = FusedRWSAdagrad(model.parameters(), lr=0.01)
    w = model.emb_l[0].embs.weight
    with pytest.raises(SystemExit, match="ERROR: the fused row-wise Adagrad update is not built for mixed-dimension embedding tables"):
        model._apply_pending([((w,), None, None, None)], opt, None)


def test_torchrec_variants_refuse_md_tables():
    """their constructors take no md_* argument; the refusal guards create_emb, which ShardedDLRM calls itself and a subclass may reach with
    md_flag set — reached here the same way"""
    import inspect
    from dlrm_amd import torchrec_variant as tv
    for cls in (tv.DLRM, tv.ShardedDLRM, tv.DLRM_DCN):
        assert not any(p.startswith("md_") or p == "kwargs" for p in inspect.signature(cls.__init__).parameters), cls.__name__
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.md_flag, m.md_threshold = True, 2
        with pytest.raises(SystemExit, match="ERROR: mixed-dimension embeddings are built for DLRM_Net only"):
            m.create_emb([8, 4], np.asarray([300, 30]))


def test_holder_refuses_a_width_above_the_base():
    from dlrm_amd.dlrm_net import PrEmbeddingBagHolder
    with pytest.raises(ValueError, match="Embedding dim 16 > base dim 8"):
        PrEmbeddingBagHolder(10, 16, 8)


def test_a_model_without_md_flag_is_the_model_it_was():
    """md_flag off: plain holders, numpy-drawn; the MD code is not reached"""
    import dlrm_amd
    case = _tiny_case()
    np.random.seed(5)
    a = dlrm_amd.DLRM_Net(8, np.asarray(case["ln_emb"]), np.asarray(case["ln_bot"]), np.asarray(case["ln_top"]), "dot")
    np.random.seed(5)
    b = dlrm_amd.DLRM_Net(8, np.asarray(case["ln_emb"]), np.asarray(case["ln_bot"]), np.asarray(case["ln_top"]), "dot", md_flag=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not b._has_md(b.emb_l)
