"""Dynamic int8 / fp16 quantised MLP towers on the device: dlrm_q8_pack_weight / dlrm_q8_quantize_act / dlrm_gemm_q8 through dlrm_amd.ops,
FusedMLP.quantize, DLRM_Net.quantize_mlp and the launcher's quantize_dynamic.

The oracle is the numpy restatement of torch's dynamic quantised Linear in tests/test_quant_mlp_host.py (pinned against torch there).
Packed weights, activation codes, parameters and the outputs of act = none / ReLU layers are compared BIT FOR BIT; sigmoid outputs and
model predictions at the project's prediction bar (rtol 2e-5 / atol 1e-6), int8 predictions under the fixture's model-level conditions.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_quant_mlp_host as H
from conftest import load_golden, params_with_prefix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MS, KS, NS = [1, 3, 65, 257, 1000], [1, 13, 64, 65, 479, 1024], [1, 3, 16, 100, 512]
ACTS = {"none": 0, "relu": 1, "sigmoid": 2}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def dev_input(x, unaligned=False):
    """x on the device; K = 479 gets the 480-wide layout of the interaction output with a NaN in the padding column (never read)"""
    M, K = x.shape
    ld = 480 if K == 479 else K
    buf = torch.full((M * ld + 1,), float("nan"), device=dev())
    view = buf[1:] if unaligned else buf[:M * ld]
    view = view.view(M, ld)
    view[:, :K] = to_dev(x)
    return view if ld != K else view[:, :K]


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("N,K", [(1, 1), (3, 13), (16, 64), (100, 65), (512, 479), (64, 1024)])
@pytest.mark.parametrize("kind", ["normal", "zero", "huge"])
def test_packed_weight_equals_the_restatement(N, K, kind):
    from dlrm_amd import ops
    rng = np.random.default_rng(N * 3 + K)
    W = (rng.standard_normal((N, K)) * 0.3).astype(f32)
    if kind == "zero":
        W[:] = 0
    elif kind == "huge":
        W[N // 2, K // 2] = 1e6
    buf = torch.empty(N * (K + 3) + 1, device=dev())[1:].view(N, K + 3)       # strided and 4-byte aligned only
    buf[:, :K] = to_dev(W)
    buf[:, K:] = float("nan")
    q = ops.q8_pack_weight(buf[:, :K])
    s, codes = H.weight_q8(W)
    got = q.codes.cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (N, H.k64(K)) and (q.N, q.K) == (N, K)
    assert np.array_equal(got[:, :K], codes) and not got[:, K:].any()
    sw = q.scale.cpu().numpy()
    assert bits(sw[0]) == bits(s) and bits(sw[1]) == bits(f32(1.0) / s)


def test_packed_fixture_weights_have_the_reference_sha():
    from dlrm_amd import ops
    d, meta = load_golden("quant_mlp_inference")
    for name, sha in meta["weight_sha256"].items():
        W = d["init." + name + ".weight"]
        q = ops.q8_pack_weight(to_dev(W))
        assert H.code_sha(q.codes.cpu().numpy()[:, :W.shape[1]]) == sha, name
        assert bits(q.scale.cpu().numpy()[0]) == bits(d["s_w." + name]), name


# ------------------------------------------------------------------------------------------------ activations
def act_inputs(kind, M, K, rng):
    x = rng.standard_normal((M, K)).astype(f32) * f32(1.7)
    if kind == "positive":
        x = np.abs(x) + f32(0.25)
    elif kind == "negative":
        x = -np.abs(x) - f32(0.25)
    elif kind == "zero":
        x[:] = 0
    elif kind == "ties":
        # s_x = 2^-4 exactly (range [-3, 127/16 - 3]), zero point 48; every value sits on a .5 code boundary: x * inv = c + 0.5 exactly
        s = f32(0.0625)
        c = rng.integers(-48, 79, size=(M, K)).astype(f32)
        x = ((c + f32(0.5)) * s).astype(f32)
        x.flat[0] = -3.0
        x.flat[-1] = f32(127 * 0.0625 - 3.0)
    return x


def check_quantise(x, unaligned=False):
    from dlrm_amd import ops
    M, K = x.shape
    X = dev_input(x, unaligned)
    codes, qp, _ = ops.q8_quantize_act(X, K)
    sx, zp, xq = H.act_q8(x)
    got, qp = codes.cpu().numpy(), qp.cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (M, H.k64(K))
    assert bits(qp[0]) == bits(sx) and qp[1] == zp and bits(qp[2]) == bits(f32(1.0) / sx), (qp, sx, zp)
    assert np.array_equal(got[:, :K].astype(np.int32), xq - zp) and not got[:, K:].any()
    return sx, zp


ACT_SHAPES = [(1, 1), (3, 13), (65, 64), (257, 65), (1000, 479), (257, 1024), (5000, 13)]


# (the tie pattern needs two elements to fix its range: no single-element case)
@pytest.mark.parametrize("kind,M,K", [(k, m, n) for k in ["signed", "positive", "negative", "zero", "ties"] for m, n in ACT_SHAPES
                                      if not (k == "ties" and m * n < 2)])
def test_quantised_activation_equals_the_restatement(kind, M, K):
    sx, zp = check_quantise(act_inputs(kind, M, K, np.random.default_rng(M + K)), unaligned=(M % 2 == 1))
    if kind == "zero":
        assert sx == f32(0.1) and zp == 0
    if kind == "ties":
        assert sx == f32(0.0625) and zp == 48
    if kind == "positive":
        assert zp == 0
    if kind == "negative":
        assert zp == 127


def test_quantise_phases_split_gives_the_same_codes():
    from dlrm_amd import ops
    x = act_inputs("signed", 300, 100, np.random.default_rng(1))
    X = to_dev(x)
    codes, qp, ws = ops.q8_quantize_act(X)
    b = (torch.zeros_like(codes), torch.zeros_like(qp), torch.zeros_like(ws))
    ops.q8_quantize_act(X, phases=ops.Q8_RANGE, bufs=b)
    ops.q8_quantize_act(X, phases=ops.Q8_QUANTIZE, bufs=b)
    assert torch.equal(b[0], codes) and torch.equal(b[1], qp)


# ------------------------------------------------------------------------------------------------ GEMM
def run_linear(x, W, b, act, strided, unaligned):
    """ops.linear_q8 into a NaN-filled buffer; returns (result, everything around it is still NaN)"""
    from dlrm_amd import ops
    M, N = x.shape[0], W.shape[0]
    q = ops.q8_pack_weight(to_dev(W))
    bias = None
    if b is not None:
        bias = torch.empty(N + 1, device=dev())[1:] if unaligned else torch.empty(N, device=dev())
        bias.copy_(to_dev(b))
    ld = N + 3 if strided else N
    buf = torch.full((M * ld + 2,), float("nan"), device=dev())
    off = 1 if (unaligned or strided) else 0
    out = buf[off:off + M * ld].view(M, ld)[:, :N]
    ops.linear_q8(dev_input(x, unaligned), q, bias, ACTS[act], out)
    full = buf.cpu().numpy()
    inner = full[off:off + M * ld].reshape(M, ld)
    canaries_ok = np.isnan(full[:off]).all() and np.isnan(full[off + M * ld:]).all() and np.isnan(inner[:, N:]).all()
    return inner[:, :N].copy(), canaries_ok


def check_linear(x, W, b, act, strided=False, unaligned=False):
    got, canaries_ok = run_linear(x, W, b, act, strided, unaligned)
    assert canaries_ok, "written outside out"
    want = H.apply_act(H.linear_q8(x, W, b), act)
    if act == "sigmoid":
        np.testing.assert_allclose(got, want, rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
    else:
        diff = bits(got) != bits(want)
        assert not diff.any(), "%d of %d outputs differ in bits (first at %s)" % (int(diff.sum()), diff.size, np.argwhere(diff)[0])
    return got


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_linear_q8_equals_the_restatement_bit_for_bit(M, K):
    rng = np.random.default_rng(M * 11 + K)
    x = (rng.standard_normal((M, K)) * 1.3).astype(f32)
    for j, N in enumerate(NS):
        W = (rng.standard_normal((N, K)) * 0.2).astype(f32)
        b = rng.standard_normal(N).astype(f32)
        act = ["none", "relu", "sigmoid"][(j + M + K) % 3]
        first = check_linear(x, W, b, act, strided=bool((j + M) % 2), unaligned=bool((j + K) % 2))
        if j % 2 == 0:
            again, _ = run_linear(x, W, b, act, bool((j + M) % 2), bool((j + K) % 2))
            assert np.array_equal(bits(first), bits(again)), "two runs differ"


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
@pytest.mark.parametrize("N", [1, 100])
def test_linear_q8_every_activation_and_no_bias(act, N):
    x, W, b = H.case(257, 65, N, seed=5, hidden=False)
    check_linear(x, W, b, act)
    check_linear(x, W, None, act, strided=True)


@pytest.mark.parametrize("N_or_M", [5, 100, 200])
def test_identity_against_an_asymmetric_matrix_both_ways(N_or_M):
    """exact small integers straight into dlrm_gemm_q8 (scales 1): out = A . B^T with A = I returns B^T, with B = I returns A — a swapped
    row / column map or a k order that differs between the operands cannot pass"""
    from dlrm_amd import ops
    K = 100
    K64 = H.k64(K)
    n = N_or_M
    asym = ((3 * np.arange(n)[:, None] + 5 * np.arange(K)[None, :]) % 11 - 5).astype(np.int8)        # [n, K], asym[i, j] != asym[j, i]
    eye = np.eye(K, dtype=np.int8)
    one = to_dev(np.asarray([1.0, 0.0, 1.0, 0.0], dtype=f32))

    def pad(a):
        out = np.zeros((a.shape[0], K64), dtype=np.int8)
        out[:, :K] = a
        return to_dev(out)

    # A = I [K, K], B = asym [n, K]: out [K, n] = asym^T
    W = ops.Q8Weight(pad(asym), to_dev(np.asarray([1.0, 1.0], dtype=f32)), n, K)
    out = torch.empty((K, n), device=dev())
    ops.gemm_q8(pad(eye), one, W, None, 0, out)
    assert np.array_equal(out.cpu().numpy(), asym.T.astype(f32))
    # A = asym [n, K], B = I [K, K]: out [n, K] = asym
    W = ops.Q8Weight(pad(eye), to_dev(np.asarray([1.0, 1.0], dtype=f32)), K, K)
    out = torch.empty((n, K), device=dev())
    ops.gemm_q8(pad(asym), one, W, None, 0, out)
    assert np.array_equal(out.cpu().numpy(), asym.astype(f32))


def test_linear_q8_at_65536_x_1024_x_1024():
    from dlrm_amd import ops
    M, K, N = 65536, 1024, 1024
    g = torch.Generator(device=dev()).manual_seed(9)
    X = torch.randn((M, K), device=dev(), generator=g)
    rng = np.random.default_rng(10)
    W = (rng.standard_normal((N, K)) * 0.03).astype(f32)
    b = rng.standard_normal(N).astype(f32)
    q = ops.q8_pack_weight(to_dev(W))
    out = ops.linear_q8(X, q, to_dev(b), 1)
    out2 = ops.linear_q8(X, q, to_dev(b), 1)
    assert torch.equal(out, out2), "two runs differ"
    rows = np.unique(np.concatenate([[0, 127, 128, M - 129, M - 1], rng.integers(0, M, size=300)]))
    sx, zp, inv = H.act_params(float(X.min()), float(X.max()))
    xs = X[to_dev(rows)].cpu().numpy()
    xq = np.clip(np.rint(xs * inv) + f32(zp), 0, 127).astype(np.int32) - zp
    s_w, wq = H.weight_q8(W)
    acc = (xq.astype(np.float64) @ wq.astype(np.float64).T).astype(np.int64)
    want = np.maximum(acc.astype(f32) * f32(sx * s_w) + b, f32(0))
    got = out[to_dev(rows)].cpu().numpy()
    assert np.array_equal(bits(got), bits(want))


def test_operators_refuse_wrong_operands():
    from dlrm_amd import ops
    q = ops.q8_pack_weight(torch.zeros((8, 20), device=dev()))
    with pytest.raises(RuntimeError, match="input width"):
        ops.linear_q8(torch.zeros((4, 19), device=dev()), q, None, 0)
    with pytest.raises(RuntimeError, match="input width"):
        ops.linear_q8(torch.zeros((4, 28), device=dev()), q, None, 0)
    codes, qp, _ = ops.q8_quantize_act(torch.zeros((4, 20), device=dev()))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gemm_q8(codes, qp, q, None, 0, torch.zeros((4, 9), device=dev()))
    with pytest.raises(RuntimeError, match="bias length"):
        ops.gemm_q8(codes, qp, q, torch.zeros(7, device=dev()), 0, torch.zeros((4, 8), device=dev()))


# ------------------------------------------------------------------------------------------------ a whole tower
def make_tower(ln, sigmoid_layer, seed):
    import dlrm_amd
    np.random.seed(seed)
    tower = dlrm_amd.DLRM_Net().create_mlp(np.asarray(ln), sigmoid_layer)
    params = {"t." + k: v.detach().numpy().copy() for k, v in tower.state_dict().items()}
    return tower.to(dev()), params


def test_bottom_tower_writes_its_slot_of_the_feature_buffer():
    from dlrm_amd.functional import OutSlot
    tower, params = make_tower([13, 64, 32, 16], -1, seed=21)
    tower.quantize(8)
    x = np.random.default_rng(22).random((300, 13)).astype(f32)
    feat = torch.full((300, 16 + 3 * 16), float("nan"), device=dev())
    with torch.enable_grad():
        y = tower(to_dev(x), out_slot=OutSlot(feat[:, :16]))
    assert y.grad_fn is None and y.data_ptr() == feat.data_ptr()
    want = H.tower_q8(x, params, "t", -1)
    got = feat.cpu().numpy()
    assert np.array_equal(bits(got[:, :16]), bits(want)) and np.isnan(got[:, 16:]).all()


def test_top_tower_reads_the_zero_padded_480_wide_input():
    tower, params = make_tower([479, 100, 64, 1], 2, seed=23)
    tower.quantize(8)
    x = (np.random.default_rng(24).standard_normal((257, 479)) * 0.7).astype(f32)
    X = torch.zeros((257, 480), device=dev())
    X[:, :479] = to_dev(x)
    got = tower(X).cpu().numpy()
    want = H.tower_q8(x, params, "t", 2)
    np.testing.assert_allclose(got, want, rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
    got479 = tower(to_dev(x)).cpu().numpy()
    assert np.array_equal(bits(got), bits(got479))


# ------------------------------------------------------------------------------------------------ model
def build_model(meta, params, **kw):
    import dlrm_amd
    np.random.seed(1)
    model = dlrm_amd.DLRM_Net(meta["m_spa"], np.asarray(meta["ln_emb"]), np.asarray(meta["ln_bot"]), np.asarray(meta["ln_top"]),
                              "dot", sigmoid_top=meta["sigmoid_top"], loss_function="bce", **kw)
    if params is not None:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return model


def forward_dev(model, X, lS_o, lS_i):
    from dlrm_amd import ops
    Z = model(to_dev(X), [to_dev(o) for o in lS_o], [to_dev(i) for i in lS_i])
    ops.check_index_errors(sync=True)
    return Z


@pytest.mark.parametrize("order", ["mlp only", "mlp then tables", "tables then mlp"])
@pytest.mark.parametrize("mlp_bits", [8, 16])
def test_model_against_the_live_reference(mlp_bits, order):
    d, meta = load_golden("quant_mlp_inference")
    model = build_model(meta, params_with_prefix(d, "init")).to(dev())
    emb_bits = 32 if order == "mlp only" else 8
    if order == "tables then mlp":
        model.quantize_embedding(8)
    model.quantize_mlp(mlp_bits)
    if order == "mlp then tables":
        model.quantize_embedding(8)                             # (the reference's order)
    assert model.quantize_mlp_bits == mlp_bits and model.bot_l.quant_bits == mlp_bits and model.top_l.quant_bits == mlp_bits
    gap = H.quarter_gap(d, emb_bits, meta["steps"])
    for s in range(meta["steps"]):
        with torch.enable_grad():
            Z = forward_dev(model, *H.fixture_batch(d, meta, s))
        assert Z.grad_fn is None and not Z.requires_grad
        H.check_model_conditions(Z.cpu().numpy(), d[f"pred_m{mlp_bits}_e{emb_bits}.s{s}"], mlp_bits, gap, "%s, step %d" % (order, s))


def onehot_case(seed, B=256, D=128):
    """one lookup per bag, D = 128: the fused lookup + interaction path"""
    rng = np.random.default_rng(seed)
    ln_emb = [300, 3, 4000]
    F = len(ln_emb) + 1
    meta = {"m_spa": D, "ln_emb": ln_emb, "ln_bot": [13, 64, D], "ln_top": [D + F * (F - 1) // 2, 64, 1], "sigmoid_top": 1}
    X = rng.random((B, 13)).astype(f32)
    return meta, X, [np.arange(B, dtype=np.int64) for _ in ln_emb], [rng.integers(0, n, size=B).astype(np.int64) for n in ln_emb]


@pytest.mark.parametrize("mlp_bits", [8, 16])
def test_model_with_fp32_tables_through_the_fused_lookup_and_interaction(mlp_bits):
    from dlrm_amd import ops
    meta, X, lS_o, lS_i = onehot_case(31)
    model = build_model(meta, None).to(dev())
    params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    model.quantize_mlp(mlp_bits)
    p0 = ops.IOTA_STATS["device_predicates"]
    with torch.enable_grad():
        Z = forward_dev(model, X, lS_o, lS_i)
    assert Z.grad_fn is None
    assert ops.IOTA_STATS["device_predicates"] == p0 + 1, "the fused path's launch predicate was not taken"
    want = H.restated_forward(params, mlp_bits, 32, X, lS_o, lS_i, sigmoid_top=1)
    # (the interaction's arithmetic differs between device and host: the same conditions as against the reference, with the effect of
    # the quantisation on THIS model as the yardstick)
    gap = 0.25 * float(np.abs(want.astype(np.float64) - H.restated_forward(params, 32, 32, X, lS_o, lS_i, sigmoid_top=1)).mean())
    H.check_model_conditions(Z.cpu().numpy(), want, mlp_bits, gap, "fused path")


@pytest.mark.parametrize("mlp_bits", [8, 16])
def test_evaluate_inference_on_a_quantised_model(mlp_bits):
    from dlrm_amd import evaluate
    d, meta = load_golden("quant_mlp_inference")
    model = build_model(meta, params_with_prefix(d, "init")).to(dev())
    model.quantize_mlp(mlp_bits)
    rng = np.random.default_rng(41)
    batches, preds, targets = [], [], []
    for s in range(meta["steps"]):
        X, lS_o, lS_i = H.fixture_batch(d, meta, s)
        Tg = np.round(rng.random((X.shape[0], 1))).astype(f32)
        batches.append((torch.from_numpy(X), [torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i], torch.from_numpy(Tg)))
        preds.append(forward_dev(model, X, lS_o, lS_i).reshape(-1))
        targets.append(Tg.reshape(-1))
    got = evaluate.inference(model, batches, device=dev())
    S, Y = torch.cat(preds).cpu().numpy(), np.concatenate(targets)
    assert got["n"] == S.size and got["tp"] + got["tn"] == int((np.round(S) == Y).sum())


# ------------------------------------------------------------------------------------------------ launcher
def _reference_dir() -> str:
    env = os.environ.get("DLRM_REFERENCE", "")
    if env and os.path.isfile(os.path.join(env, "dlrm_s_pytorch.py")):
        return env
    from oracle.build_ref import ref_dir
    return ref_dir() or ""


_REF = _reference_dir()


@pytest.mark.skipif(not _REF, reason="no reference: neither $DLRM_REFERENCE nor a usable oracle/_ref (run `make -C oracle ref` where a "
                                     "checkout exists)")
def test_launcher_with_quantize_mlp_matches_the_reference_cpu_run(tmp_path):
    """the UNMODIFIED reference CLI with --inference-only --quantize-mlp-with-bit 8: through dlrm_amd.launch on the GPU, and as it is on the
    CPU (identical seeds: identical parameters and data).  The inference-only run reports one accuracy line and no loss."""
    cli = ["--arch-sparse-feature-size=16", "--arch-mlp-bot=13-32-16", "--arch-mlp-top=31-32-1", "--arch-embedding-size=60-3-500-1200-250",
           "--mini-batch-size=64", "--data-size=512", "--num-batches=8", "--num-indices-per-lookup=3", "--numpy-rand-seed=123",
           "--loss-function=bce", "--round-targets=True", "--inference-only", "--quantize-mlp-with-bit=8"]
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
    pat = re.compile(r"accuracy ([\d.]+) %, best ([\d.]+) %")
    lo, lr_ = pat.findall(ours.stdout), pat.findall(ref.stdout)
    print("launcher: ", lo, "\nreference:", lr_)
    assert len(lo) == 1 and len(lr_) == 1, (ours.stdout[-1500:], ref.stdout[-1500:])
    for a, b in zip(lo[0], lr_[0]):
        assert abs(float(a) - float(b)) <= H.PRED_ATOL + H.PRED_RTOL * abs(float(b)), (lo, lr_)
    assert "Testing for inference only" in ours.stdout


# ------------------------------------------------------------------------------------------------ refusals, and the old branch
def quantised_tiny(bits=8):
    meta, X, lS_o, lS_i = onehot_case(51, B=64, D=16)
    model = build_model(meta, None).to(dev())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.quantize_mlp(bits)
    return model, opt, (X, lS_o, lS_i)


@pytest.mark.parametrize("bits", [8, 16])
def test_stepping_an_optimizer_over_quantised_towers_is_refused(bits):
    model, opt, _ = quantised_tiny(bits)
    with pytest.raises(SystemExit, match="ERROR: this optimizer holds the parameters of MLP towers that are quantized now"):
        opt.step()
    torch.optim.SGD(model.emb_l.parameters(), lr=0.1).step()                  # the tables alone may still step


def test_quantising_twice_is_refused():
    model, _, batch = quantised_tiny(8)
    before = forward_dev(model, *batch).clone()
    with pytest.raises(SystemExit, match="ERROR: the MLP towers are quantized already \\(8 bits\\)"):
        model.quantize_mlp(16)
    assert torch.equal(forward_dev(model, *batch), before)


def test_moving_or_loading_into_a_quantised_model_is_refused_unchanged():
    model, _, batch = quantised_tiny(8)
    before = forward_dev(model, *batch).clone()
    state = {k: v.clone() + 1 for k, v in model.state_dict().items()}
    with pytest.raises(SystemExit, match="ERROR: a model with quantized MLP towers \\(8 bits\\) cannot be moved or converted"):
        model.to("cpu")
    with pytest.raises(SystemExit, match="ERROR: a quantized MLP tower \\(8 bits\\) cannot be moved or converted"):
        model.top_l.cpu()
    with pytest.raises(SystemExit, match="ERROR: load_state_dict into a model with quantized MLP towers \\(8 bits\\)"):
        model.load_state_dict(state)
    assert all(v.is_cuda for v in model.state_dict().values())
    assert torch.equal(forward_dev(model, *batch), before)


def test_an_md_model_is_refused_unchanged():
    import dlrm_amd
    np.random.seed(6)
    model = dlrm_amd.DLRM_Net(np.asarray([16, 4, 8]), np.asarray([40, 300, 200]), np.asarray([13, 32, 16]), np.asarray([16 + 6, 32, 1]), "dot",
                              sigmoid_top=1, md_flag=True, md_threshold=2).to(dev())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(SystemExit, match="ERROR: quantized MLP towers with mixed dimensions are not supported"):
        model.quantize_mlp(8)
    assert model.quantize_mlp_bits == 32 and all(torch.equal(model.state_dict()[k], before[k]) for k in before)


def test_graphed_train_step_refuses_quantised_towers():
    from dlrm_amd.graph import GraphedTrainStep
    model, _, _ = quantised_tiny(16)
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep captures a training step; a model with quantized MLP towers"):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1))


@pytest.mark.parametrize("arith", ["f32", "bf16"])
def test_quantize_mlp_32_changes_nothing_in_a_training_step(arith):
    """quantize_mlp(32) is a no-op on the device too: forward, backward and update of a deterministic-mode step from the same parameters
    give the same bits whether it was called or not, with an autograd node, and the f32 predictions are the golden ones of the fixture at the
    project's bar.  (That an unquantised model gives the bits it gave BEFORE this feature existed is what the unchanged older suites show,
    not this test: both legs here run the new code.)"""
    from dlrm_amd import ops
    d, meta = load_golden("config1_b128")
    T = len(meta["ln_emb"])
    results = []
    for noop_call in (False, True):
        model = build_model(meta, params_with_prefix(d, "init")).to(dev())
        model.set_mlp_arith(arith)
        model.emb_update_mode = ops.UPD_DETERMINISTIC
        if noop_call:
            model.quantize_mlp(32)
        assert model.quantize_mlp_bits == 32
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        Z = model(to_dev(d["s0.X"]), [to_dev(d[f"s0.off{k}"]) for k in range(T)], [to_dev(d[f"s0.idx{k}"]) for k in range(T)])
        assert Z.grad_fn is not None
        E = model.loss_fn(Z, to_dev(d["s0.T"]))
        opt.zero_grad()
        E.backward()
        opt.step()
        torch.cuda.synchronize()
        results.append((Z.detach().clone(), {k: v.clone() for k, v in model.state_dict().items()}))
    assert torch.equal(results[0][0], results[1][0])
    assert all(torch.equal(results[0][1][k], results[1][1][k]) for k in results[0][1])
    if arith == "f32":
        np.testing.assert_allclose(results[0][0].cpu().numpy(), d["s0.Z"], rtol=H.PRED_RTOL, atol=H.PRED_ATOL)
