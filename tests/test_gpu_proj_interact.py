"""The projected interaction of DLRM_Projection on the GPU: dlrm_proj_interact_fwd / _bwd (csrc/interact_proj.hip) against an fp64 numpy
evaluation of the formulas in include/dlrm_hip.h, functional.ProjectInteractFunction against torch autograd of bmm + cat, and
torchrec_variant.DLRM_Projection against the same model composed of torch CPU operators (torchrec itself is absent: UNPINNED).

Tolerances are the project's own for a 128-term fp32 dot of N(0, 1) data (test_interact_fwd_bwd): forward rtol 1e-5 with atol 1e-5 for
B <= 67 and 3e-5 above, backward twice that atol."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# (I1, I2, D): the trainer's defaults at D = 128 / 64; asymmetric ones (a row / column swap shows); the smallest; D % 4 != 0 and I1 > 32 take the
# generic kernels
SHAPES = [(16, 16, 128), (32, 32, 64), (16, 8, 128), (3, 5, 12), (1, 1, 4), (2, 7, 6), (33, 2, 8)]
BATCHES = [1, 67, 2051]


def _r4(n):
    return (n + 3) & ~3


def _atol(B):
    return 1e-5 if B <= 67 else 3e-5


def _ref_fwd(x, P1, P2, I1, I2, D):
    B = x.shape[0]
    Z = np.einsum("bid,bdj->bij", P1.astype(np.float64).reshape(B, I1, D), P2.astype(np.float64).reshape(B, D, I2))
    return np.concatenate([x.astype(np.float64), Z.reshape(B, I1 * I2)], axis=1)


def _ref_bwd(P1, P2, dR, I1, I2, D):
    B = P1.shape[0]
    A, Bm = P1.astype(np.float64).reshape(B, I1, D), P2.astype(np.float64).reshape(B, D, I2)
    dZ = dR[:, D:D + I1 * I2].astype(np.float64).reshape(B, I1, I2)
    dA = np.einsum("bij,bdj->bid", dZ, Bm)
    dBm = np.einsum("bid,bij->bdj", A, dZ)
    return dR[:, :D].astype(np.float64), dA.reshape(B, I1 * D), dBm.reshape(B, D * I2)


def _inputs(rng, B, I1, I2, D, ints=False):
    def draw(*shape):
        if ints:
            return rng.integers(-4, 5, size=shape).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)
    return draw(B, D), draw(B, I1 * D), draw(B, D * I2), draw(B, _r4(D + I1 * I2))


def _run(x, P1, P2, dR, D, ldr):
    """forward into an R pre-filled with 3.0, backward into outputs pre-filled with 3.0 (operands are torch GPU tensors, possibly strided)"""
    from dlrm_amd import ops
    B = x.size(0)
    R = torch.full((B, ldr), 3.0, dtype=torch.float32, device=x.device)
    ops.proj_interact_fwd(x, P1, P2, D, R)
    dx, dP1, dP2 = (torch.full(s, 3.0, dtype=torch.float32, device=x.device) for s in ((B, D), tuple(P1.shape), tuple(P2.shape)))
    ops.proj_interact_bwd(P1, P2, D, dR, dx, dP1, dP2)
    return R, dx, dP1, dP2


def _check(got, x, P1, P2, dR, I1, I2, D, B):
    R, dx, dP1, dP2 = (t.cpu().numpy() for t in got)
    W = D + I1 * I2
    want = _ref_fwd(x, P1, P2, I1, I2, D)
    assert np.array_equal(R[:, :D], x)
    assert np.array_equal(R[:, W:], np.zeros((B, R.shape[1] - W), dtype=np.float32))
    np.testing.assert_allclose(R[:, D:W], want[:, D:], rtol=1e-5, atol=_atol(B))
    wdx, wdP1, wdP2 = _ref_bwd(P1, P2, dR, I1, I2, D)
    assert np.array_equal(dx, dR[:, :D])
    np.testing.assert_allclose(dP1, wdP1, rtol=1e-5, atol=2 * _atol(B))
    np.testing.assert_allclose(dP2, wdP2, rtol=1e-5, atol=2 * _atol(B))


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("I1,I2,D", SHAPES)
def test_kernels_match_fp64_formulas(I1, I2, D, B):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 * I1 + 10 * I2 + D + B)
    x, P1, P2, dR = _inputs(rng, B, I1, I2, D)
    got = _run(*(torch.from_numpy(a).to(dev) for a in (x, P1, P2, dR)), D, dR.shape[1])
    _check(got, x, P1, P2, dR, I1, I2, D, B)


@gpu
@pytest.mark.parametrize("I1,I2,D", [(16, 8, 128), (3, 5, 12)])
def test_layout_is_exact_on_small_integers(I1, I2, D):
    """integers in [-4, 4]: every product and every partial sum is an integer below 2^24, so fp32 is exact in any order and a wrong index anywhere
    changes the result"""
    dev = torch.device("cuda:0")
    B = 67
    rng = np.random.default_rng(5)
    x, P1, P2, dR = _inputs(rng, B, I1, I2, D, ints=True)
    R, dx, dP1, dP2 = (t.cpu().numpy() for t in _run(*(torch.from_numpy(a).to(dev) for a in (x, P1, P2, dR)), D, dR.shape[1]))
    W = D + I1 * I2
    want = _ref_fwd(x, P1, P2, I1, I2, D)
    assert np.array_equal(R[:, :W].astype(np.float64), want)
    assert np.array_equal(R[:, W:], np.zeros((B, R.shape[1] - W), dtype=np.float32))
    wdx, wdP1, wdP2 = _ref_bwd(P1, P2, dR, I1, I2, D)
    assert np.array_equal(dx.astype(np.float64), wdx)
    assert np.array_equal(dP1.astype(np.float64), wdP1)
    assert np.array_equal(dP2.astype(np.float64), wdP2)


@gpu
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "x-off-by-one"])
@pytest.mark.parametrize("I1,I2,D", [(16, 16, 128), (3, 5, 12)])
def test_strided_and_unaligned_operands(I1, I2, D, shift):
    """x is a column slice of a wider buffer (x_ld = 5 * D), P1 / P2 / dR and the gradients have padded leading dimensions; with shift = 1
    x starts one element into its buffer: 4-byte alignment only, which the LDS kernel does not take"""
    dev = torch.device("cuda:0")
    B = 67
    rng = np.random.default_rng(77 + shift)
    x, P1, P2, dR = _inputs(rng, B, I1, I2, D)
    W = D + I1 * I2

    def padded(a, extra, fill=7.0):
        buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=dev)
        buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
        return buf[:, :a.shape[1]]
    xbuf = torch.full((B * 5 * D + 4,), 7.0, dtype=torch.float32, device=dev)
    xv = xbuf[shift:shift + B * 5 * D].view(B, 5 * D)[:, :D]
    xv.copy_(torch.from_numpy(x).to(dev))
    assert xv.stride(0) == 5 * D and (xv.data_ptr() % 16 == 0) == (shift == 0)
    P1v, P2v, dRv = padded(P1, 8), padded(P2, 12), padded(dR, 4)
    from dlrm_amd import ops
    Rv = torch.full((B, _r4(W)), 3.0, dtype=torch.float32, device=dev)
    ops.proj_interact_fwd(xv, P1v, P2v, D, Rv)
    outs = [torch.full((B, w + 4), 3.0, dtype=torch.float32, device=dev) for w in (D, I1 * D, D * I2)]
    dxv, dP1v, dP2v = (o[:, :o.size(1) - 4] for o in outs)
    ops.proj_interact_bwd(P1v, P2v, D, dRv, dxv, dP1v, dP2v)
    _check((Rv, dxv, dP1v, dP2v), x, P1, P2, dR, I1, I2, D, B)
    # the inputs are unchanged and nothing beyond the gradient views was written
    assert bool((xbuf.view(-1)[shift:shift + B * 5 * D].view(B, 5 * D)[:, D:] == 7.0).all())
    assert all(bool((o[:, -4:] == 3.0).all()) for o in outs)


@gpu
def test_batch_independence_and_determinism():
    dev = torch.device("cuda:0")
    I1, I2, D, B = 16, 16, 128, 67
    rng = np.random.default_rng(3)
    ops_in = [torch.from_numpy(a).to(dev) for a in _inputs(rng, B, I1, I2, D)]
    ldr = ops_in[3].size(1)
    first = _run(*ops_in, D, ldr)
    again = _run(*ops_in, D, ldr)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    head = _run(*(t[:5].contiguous() for t in ops_in), D, ldr)
    for a, b in zip(first, head):
        assert torch.equal(a[:5], b)


@gpu
def test_argument_checks_raise_before_any_launch():
    from dlrm_amd import ops
    dev = torch.device("cuda:0")
    B, D, I1, I2 = 4, 8, 2, 3

    def z(*shape, device=dev):
        return torch.zeros(shape, dtype=torch.float32, device=device)
    with pytest.raises(RuntimeError, match="dlrm_amd: proj_interact_fwd shape mismatch"):          # I1 = 0
        ops.proj_interact_fwd(z(B, D), z(B, 0), z(B, D * I2), D, z(B, 16))
    with pytest.raises(RuntimeError, match="dlrm_amd: proj_interact_fwd shape mismatch"):          # ldr < D + I1 * I2
        ops.proj_interact_fwd(z(B, D), z(B, I1 * D), z(B, D * I2), D, z(B, D + I1 * I2 - 1))
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.proj_interact_fwd(z(B, D, device="cpu"), z(B, I1 * D), z(B, D * I2), D, z(B, 16))
    with pytest.raises(RuntimeError, match="dlrm_amd: proj_interact_bwd shape mismatch"):          # I1 = 0
        ops.proj_interact_bwd(z(B, 0), z(B, D * I2), D, z(B, 16), z(B, D), z(B, 0), z(B, D * I2))
    with pytest.raises(RuntimeError, match="dlrm_amd: proj_interact_bwd shape mismatch"):          # ldr < D + I1 * I2
        ops.proj_interact_bwd(z(B, I1 * D), z(B, D * I2), D, z(B, D + I1 * I2 - 1), z(B, D), z(B, I1 * D), z(B, D * I2))
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        ops.proj_interact_bwd(z(B, I1 * D), z(B, D * I2), D, z(B, 16, device="cpu"), z(B, D), z(B, I1 * D), z(B, D * I2))
    # the library's own checks (reached past the wrapper): DLRM_E_ARG, no launch
    import ctypes as C
    from dlrm_amd import _lib
    lib = _lib.load()
    a = z(B, 64)
    p = C.c_void_p(a.data_ptr())
    assert lib.dlrm_proj_interact_fwd(B, D, 0, I2, p, D, p, 0, p, D * I2, p, 16, None) == -1
    assert lib.dlrm_proj_interact_fwd(B, D, I1, I2, p, D, p, I1 * D, p, D * I2, p, D + I1 * I2 - 1, None) == -1
    assert lib.dlrm_proj_interact_fwd(B, D, I1, I2, None, D, p, I1 * D, p, D * I2, p, 16, None) == -1
    assert lib.dlrm_proj_interact_bwd(B, 0, I1, I2, p, I1 * D, p, D * I2, p, 16, p, D, p, I1 * D, p, D * I2, None) == -1
    assert lib.dlrm_proj_interact_bwd(B, D, I1, I2, p, I1 * D, p, D * I2, p, 16, p, D - 1, p, I1 * D, p, D * I2, None) == -1
    assert lib.dlrm_proj_interact_bwd(B, D, I1, I2, p, I1 * D, p, D * I2, p, 16, p, D, None, I1 * D, p, D * I2, None) == -1
    # B = 0: empty outputs, nothing launched
    R = ops.proj_interact_fwd(z(0, D), z(0, I1 * D), z(0, D * I2), D, z(0, 16))
    assert tuple(R.shape) == (0, 16)
    dx, dP1, dP2 = z(0, D), z(0, I1 * D), z(0, D * I2)
    ops.proj_interact_bwd(z(0, I1 * D), z(0, D * I2), D, z(0, 16), dx, dP1, dP2)
    assert dx.numel() == dP1.numel() == dP2.numel() == 0
    torch.cuda.synchronize()


@gpu
def test_function_backward_matches_torch_autograd_of_bmm_and_cat():
    """(not gradcheck: the kernels are fp32)"""
    from dlrm_amd.functional import ProjectInteractFunction
    dev = torch.device("cuda:0")
    I1, I2, D, B = 3, 5, 12, 67
    rng = np.random.default_rng(9)
    x, P1, P2, _ = _inputs(rng, B, I1, I2, D)
    W = D + I1 * I2
    G = rng.standard_normal((B, _r4(W))).astype(np.float32)
    cpu = [torch.from_numpy(a).requires_grad_(True) for a in (x, P1, P2)]
    Rc = torch.cat([cpu[0], torch.bmm(cpu[1].view(B, I1, D), cpu[2].view(B, D, I2)).view(B, -1)], dim=1)
    Rc.backward(torch.from_numpy(G[:, :W]))
    gpu = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (x, P1, P2)]
    Rp = ProjectInteractFunction.apply(D, True, *gpu)
    assert tuple(Rp.shape) == (B, _r4(W))
    Ru = ProjectInteractFunction.apply(D, False, *gpu)
    assert tuple(Ru.shape) == (B, W) and torch.equal(Ru, Rp[:, :W])
    np.testing.assert_allclose(Rp[:, :W].detach().cpu().numpy(), Rc.detach().numpy(), rtol=1e-5, atol=_atol(B))
    assert bool((Rp[:, W:] == 0).all())
    Rp.backward(torch.from_numpy(G).to(dev))
    for g, c in zip(gpu, cpu):
        np.testing.assert_allclose(g.grad.cpu().numpy(), c.grad.numpy(), rtol=1e-5, atol=2 * _atol(B))
    assert torch.equal(gpu[0].grad.cpu(), torch.from_numpy(G[:, :D]))


# ------------------------------------------------------------------------------------------------ the model
ROWS, MD, MB, HOT = [40, 9, 300], 16, 48, [2, 1, 4]
MODEL_SEED, DATA_SEED = 2, 12


def _build_model():
    from dlrm_amd.torchrec_variant import DLRM_Projection
    np.random.seed(MODEL_SEED)
    return DLRM_Projection(ROWS, MD, 13, [24, MD], [32, 1], [32, 32], [24, 48])


def _batches(steps):
    rng = np.random.default_rng(DATA_SEED)
    out = []
    for _ in range(steps):
        X = torch.from_numpy(rng.random((MB, 13)).astype(np.float32))
        idx = [torch.from_numpy(rng.integers(0, n, size=MB * h)) for n, h in zip(ROWS, HOT)]
        off = [torch.arange(MB) * h for h in HOT]
        T = torch.from_numpy(rng.integers(0, 2, size=(MB, 1)).astype(np.float32))
        out.append((X, idx, off, T))
    return out


def _torch_composition(ref, X, idx, off, T):
    """DLRM_Projection of torch CPU operators over the parameter dict `ref` (fp32 or fp64): (logits, loss)"""
    import torch.nn.functional as Fn
    dt = ref["bot_l.0.weight"].dtype
    x = X.to(dt)
    for i in range(2):
        x = torch.relu(Fn.linear(x, ref[f"bot_l.{2 * i}.weight"], ref[f"bot_l.{2 * i}.bias"]))
    ly = [Fn.embedding_bag(idx[k], ref[f"emb_l.{k}.weight"], off[k], mode="sum", sparse=False) for k in range(3)]
    Cc = torch.cat([x] + ly, dim=1)
    P = []
    for name in ("proj1_l", "proj2_l"):
        p = Cc
        for i in range(2):
            p = torch.relu(Fn.linear(p, ref[f"{name}.{2 * i}.weight"], ref[f"{name}.{2 * i}.bias"]))
        P.append(p)
    B = X.size(0)
    Z = torch.bmm(P[0].view(B, -1, MD), P[1].view(B, MD, -1))
    R = torch.cat([x, Z.view(B, -1)], dim=1)
    z = torch.relu(Fn.linear(R, ref["top_l.0.weight"], ref["top_l.0.bias"]))
    logits = Fn.linear(z, ref["top_l.2.weight"], ref["top_l.2.bias"])
    return logits, Fn.binary_cross_entropy_with_logits(logits, T.to(dt))


def _train_composition(dtype, batches):
    ref = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in _build_model().state_dict().items()}
    ropt = torch.optim.SGD(list(ref.values()), lr=0.2)
    trace = []
    for X, idx, off, T in batches:
        logits, loss = _torch_composition(ref, X, idx, off, T)
        trace.append((logits.detach().clone(), float(loss.detach())))
        ropt.zero_grad(); loss.backward(); ropt.step()
    return ref, trace


@pytest.fixture(scope="module")
def composition():
    batches = _batches(2)
    return batches, _train_composition(torch.float32, batches), _train_composition(torch.float64, batches)


def test_the_fp32_composition_is_within_a_quarter_of_every_bound_of_fp64(composition):
    """the condition on the committed seed and scale: the yardstick's own fp32 error leaves three quarters of each bound to the model under test"""
    _, (ref32, tr32), (ref64, tr64) = composition
    for (l32, e32), (l64, e64) in zip(tr32, tr64):
        err = (l32.double() - l64).abs()
        assert bool((err <= 0.25 * (5e-6 + 5e-5 * l64.abs())).all()), float(err.max())
        assert abs(e32 - e64) <= 0.25 * 1e-5 * abs(e64)
    for k in ref32:
        err = (ref32[k].detach().double() - ref64[k].detach()).abs()
        assert bool((err <= 0.25 * (1e-5 + 2e-4 * ref64[k].detach().abs())).all()), (k, float(err.max()))


@gpu
def test_dlrm_projection_trains_like_a_torch_composition(composition):
    """2 FusedSGD steps (lr 0.2) against the same model composed of torch CPU operators with autograd; bounds of
    test_dlrm_dcn_model_trains_like_a_torch_composition"""
    from dlrm_amd.optim import FusedSGD
    device = torch.device("cuda:0")
    batches, (ref, trace), _ = composition
    model = _build_model().to(device)
    opt = FusedSGD(model.parameters(), lr=0.2)
    for (X, idx, off, T), (rl, RE) in zip(batches, trace):
        logits = model(X.to(device), [o.to(device) for o in off], [i.to(device) for i in idx])
        E = model.loss_fn(logits, T.to(device))
        np.testing.assert_allclose(logits.detach().cpu().numpy(), rl.numpy(), rtol=5e-5, atol=5e-6)
        assert abs(float(E.detach()) - RE) <= 1e-5 * abs(RE)
        opt.zero_grad(); E.backward(); opt.step()
    sd = model.state_dict()
    for k, v in ref.items():
        np.testing.assert_allclose(sd[k].cpu().numpy(), v.detach().numpy(), rtol=2e-4, atol=1e-5, err_msg=k)


@gpu
def test_dlrm_train_wraps_the_projection_model(composition):
    from dlrm_amd.torchrec_variant import DLRMTrain
    device = torch.device("cuda:0")
    batches, (_, trace), _ = composition
    X, idx, off, T = batches[0]
    wrapped = DLRMTrain(_build_model()).to(device)
    loss, (loss_d, logits, labels) = wrapped(X.to(device), [o.to(device) for o in off], [i.to(device) for i in idx], T.to(device))
    assert loss.requires_grad and not loss_d.requires_grad and not logits.requires_grad
    assert float(loss_d) == float(loss.detach()) and torch.equal(labels.cpu(), T)
    assert abs(float(loss.detach()) - trace[0][1]) <= 1e-5 * abs(trace[0][1])
    np.testing.assert_allclose(logits.cpu().numpy(), trace[0][0].numpy(), rtol=5e-5, atol=5e-6)
