"""Every row of tests/gemm_route_cases.py on the device: the library is first ASKED which kernel the call will launch on the real operands
(dlrm_linear_*_route — the same host code the call runs) and must name the variant the table pins; then the call runs and is checked
against the float64 oracle at the project's per-layer bars (those of tests/test_gpu_kernels.py::test_linear_fwd_bwd; the plain-bf16 rows:
those of ::test_linear_bf16_arithmetic, a float64 product of the bf16-rounded operands).

The reference, exactly: the PRODUCT (X.W^T, dY.W, dY^T.X) is the host oracle's O.linear_fwd without bias or activation — float64
accumulation, its result ROUNDED TO fp32 (2^-24 relative, far inside the bars) — or, above HOST_WORK multiply-adds, torch.matmul in
float64 on the device.  Bias, activation, the mask derivative, the accumulate prior and the bias gradient (a float64 column sum) are
restated here in torch float64 on top of that product; O.linear_bwd is not used (it applies the OUTPUT's activation derivative, where
dlrm_linear_bwd_data masks with the INPUT's, and it always computes all three gradients).  The ReLU mask and the sign bits come from the
GPU's own forward output, as in test_linear_fwd_bwd.

Every operand lives inside a larger allocation.  Outputs: the logical extent is pre-filled with NaN (none may remain), the columns up to
the pitch, four rows before and after, the sign-bit words of a band before and two behind hold a sentinel that must survive.  Inputs: pitch
padding and guard rows are NaN — include/dlrm_hip.h promises nothing about them, so a kernel that lets them reach a stored value fails its
oracle check; the one region the header DOES specify (columns K_store..K-1 of a padded weight-gradient X: zeros) is kept zero.

Bit-for-bit: a workspace weight gradient run twice; the pairs of gemm_route_cases.EQUIVALENT (straight-line epilogue = general epilogue through
a bias 4 bytes off a 16-byte boundary; sign bits = fp32 mask in the data gradient).
"""
import numpy as np
import pytest
import torch

import gemm_route_cases as G
from gemm_route_cases import DGRAD, FWD, WGRAD
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 4                  # sentinel / poison rows in front of and behind every operand
SENT = -777.25             # sentinel of output padding (a value no result takes)
BITS_SENT = 0x5A5A5A5A
HOST_WORK = 1e9            # multiply-adds above which the float64 reference product runs on the device (torch.matmul) instead of the host oracle


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


class Buf:
    """a [rows, cols] fp32 view at pitch `ld`, `off` bytes past a 16-byte boundary, inside a larger 1-D allocation filled with `fill`"""

    def __init__(self, rows, cols, ld, off, fill):
        assert off % 4 == 0 and ld >= cols
        self.rows, self.cols, self.ld = rows, cols, ld
        self.start = GUARD * ld + 4 + off // 4                     # (the allocation itself starts on a 256-byte boundary)
        self.all = torch.full(((rows + 2 * GUARD) * ld + 16,), fill, device=dev())
        assert self.all.data_ptr() % 16 == 0
        self.view = self.all.as_strided((rows, cols), (ld, 1), self.start)
        assert self.view.data_ptr() % 16 == off

    def outside_is(self, value):
        """everything but the logical extent still holds `value`"""
        chk = self.all.clone()
        chk.as_strided((self.rows, self.cols), (self.ld, 1), self.start).fill_(value)
        return bool(torch.all(chk == value))


def in_buf(c, op, data):
    """an input operand: data inside NaN-poisoned padding"""
    rows, cols = data.shape
    b = Buf(rows, cols, G.ld_of(c, op), G.off_of(c, op), float("nan"))
    b.view.copy_(data)
    return b


def out_buf(c, op, prior=None):
    """an output operand: NaN inside (or the prior values of an accumulating call), the sentinel around it"""
    rows, cols = G.operands(c)[op]
    b = Buf(rows, cols, G.ld_of(c, op), G.off_of(c, op), SENT)
    if prior is None:
        b.view.fill_(float("nan"))
    else:
        b.view.copy_(prior)
    return b


def vec_buf(c, op, data=None, n=None, fill=float("nan")):
    """a vector (bias, bias gradient) with 8 elements of padding on either side"""
    n = n if data is None else data.numel()
    off = G.off_of(c, op)
    allb = torch.full((n + 16,), fill, device=dev())
    v = allb[4 + off // 4: 4 + off // 4 + n]
    assert v.data_ptr() % 16 == off
    if data is not None:
        v.copy_(data)
    return allb, v


class Bits:
    """the sign-bit buffer of an [M, N] activation between one sentinel band in front and two behind"""

    def __init__(self, M, N):
        from dlrm_amd import _lib
        self.M, self.N, self.nblk = M, N, (N + 63) // 64
        self.words = int(_lib.load().dlrm_relu_bits_bytes(M, N)) // 4
        self.band = self.nblk * 64
        assert self.words == ((M + 31) // 32) * self.band
        self.all = torch.full((self.words + 3 * self.band,), BITS_SENT, dtype=torch.int32, device=dev())
        self.view = self.all[self.band: self.band + self.words]
        assert self.view.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool(torch.all(self.all[:self.band] == BITS_SENT)) and bool(torch.all(self.all[self.band + self.words:] == BITS_SENT))

    def decode(self):
        """[M, N] bool from the documented layout (include/dlrm_hip.h): bit 31 - (4*it + c) of word l of block (mb, nb) is element
        (32*mb + 4*it + l/16, 64*nb + 4*(l%16) + c)"""
        mbands = (self.M + 31) // 32
        w = self.view.view(mbands, self.nblk, 64, 1)
        sh = 31 - torch.arange(32, device=dev(), dtype=torch.int32)
        e = ((w >> sh) & 1).bool().view(mbands, self.nblk, 4, 16, 8, 4)            # [mb, nb, l/16, l%16, it, c]
        e = e.permute(0, 4, 2, 1, 3, 5).reshape(mbands * 32, self.nblk * 64)        # rows (mb, it, l/16), columns (nb, l%16, c)
        return e[:self.M, :self.N]


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, device=dev(), dtype=torch.float32)


def seeded(c):
    g = torch.Generator(device=dev())
    g.manual_seed(1000003 * c.M + 1009 * c.N + c.K + {FWD: 0, DGRAD: 1, WGRAD: 2}[c.entry])       # (pairs of EQUIVALENT share their data)
    return g


def rb(t):
    """fp32 -> bf16 (nearest even) -> fp32: the operand rounding of arith "bf16" """
    return t.to(torch.bfloat16).to(torch.float32)


def product64(A, B, work):
    """A [m, k] . B [n, k]^T in float64: the host oracle (O.linear_fwd) where it takes well under a second, torch.matmul on the device above"""
    if work <= HOST_WORK:
        return torch.from_numpy(O.linear_fwd(A.cpu().numpy(), B.cpu().numpy(), None, 0).astype(np.float64)).to(dev())
    return A.double() @ B.double().t()


def close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got.double().cpu().numpy(), want.cpu().numpy(), rtol=rtol, atol=atol, err_msg=what)


def check_route(c, addr):
    got = G.query(c, addr)
    assert tuple(got) == G.EXPECT[c.name], "the library would launch %r, the table pins %r" % (got, G.EXPECT[c.name])
    return got


_kept = {}       # results of the rows named in EQUIVALENT, for the bit-for-bit comparison
_PAIRED = {n for p in G.EQUIVALENT for n in p}


def activation_from_forward(c, gen, act):
    """Xact [M, K] = the GPU's own forward output of a previous layer (16 inputs), with the sign bits that forward wrote"""
    from dlrm_amd import ops
    X0, W0, b0 = randn(gen, c.M, 16), randn(gen, c.K, 16) / 4.0, randn(gen, c.K)
    Y = torch.empty((c.M, c.K), device=dev())
    bits = Bits(c.M, c.K) if act == G.RELU else None
    ops.linear_fwd(X0, W0, b0, act, Y, relu_bits=bits.view if bits is not None else None)
    torch.cuda.synchronize()
    if bits is not None:
        assert torch.equal(bits.decode(), Y > 0) and bits.guards_intact()
    return Y, bits


def run_fwd(c):
    from dlrm_amd import ops
    gen = seeded(c)
    X, W, b = randn(gen, c.M, c.K), randn(gen, c.N, c.K) / float(np.sqrt(c.K)), randn(gen, c.N)
    xb, wb = in_buf(c, "x", X), in_buf(c, "w", W)
    ball, bv = vec_buf(c, "bias", b) if c.bias else (None, None)
    yb = out_buf(c, "y")
    bits = Bits(c.M, c.N) if c.mask == "bits" else None
    addr = {"x": xb.view.data_ptr(), "w": wb.view.data_ptr(), "bias": bv.data_ptr() if c.bias else None, "y": yb.view.data_ptr(),
            "bits": bits.view.data_ptr() if bits is not None else None}
    check_route(c, addr)
    ops.linear_fwd(xb.view, wb.view, bv, c.act, yb.view, c.arith, relu_bits=bits.view if bits is not None else None)
    torch.cuda.synchronize()
    Y = yb.view
    assert not bool(torch.isnan(Y).any()), "NaN left inside the output"
    assert yb.outside_is(SENT), "the forward wrote outside Y[M, N]"
    if c.arith == "bf16":
        want, tol = product64(rb(X), rb(W), c.M * c.N * c.K), 2e-5
    else:
        want, tol = product64(X, W, c.M * c.N * c.K), 1e-5
    if c.bias:
        want = want + b.double()
    want = torch.relu(want) if c.act == G.RELU else torch.sigmoid(want) if c.act == G.SIGMOID else want
    close(Y, want, tol, tol, c.name + " Y")
    if bits is not None:
        assert torch.equal(bits.decode(), Y > 0), "sign bits differ from the output they describe"
        assert bits.guards_intact(), "sign-bit words outside the bands of M rows were written"
    if c.name in _PAIRED:
        _kept[c.name] = Y.clone()


def run_dgrad(c):
    from dlrm_amd import ops
    gen = seeded(c)
    dY, W = randn(gen, c.M, c.N), randn(gen, c.N, c.K) / float(np.sqrt(c.K))
    masked = c.mask != "none"
    Xact, bits = activation_from_forward(c, gen, c.act) if masked else (None, None)
    dyb, wb = in_buf(c, "dy", dY), in_buf(c, "w", W)
    xab = in_buf(c, "xact", Xact) if masked else None
    dxb = out_buf(c, "dx")
    use_bits = c.mask == "bits"
    addr = {"dy": dyb.view.data_ptr(), "w": wb.view.data_ptr(), "xact": xab.view.data_ptr() if masked else None, "dx": dxb.view.data_ptr(),
            "bits": bits.view.data_ptr() if use_bits else None}
    check_route(c, addr)
    ops.linear_bwd_data(dyb.view, wb.view, xab.view if masked else None, c.act if masked else 0, dxb.view, c.arith,
                        relu_bits=bits.view if use_bits else None)
    torch.cuda.synchronize()
    dX = dxb.view
    assert not bool(torch.isnan(dX).any()), "NaN left inside the output"
    assert dxb.outside_is(SENT), "the data gradient wrote outside dX[M, K]"
    Wt = W.t().contiguous()
    if c.arith == "bf16":
        want, tol = product64(rb(dY), rb(Wt), c.M * c.N * c.K), 2e-5
    else:
        want, tol = product64(dY, Wt, c.M * c.N * c.K), 1e-5
    if masked:
        xa = Xact.double()
        want = want * ((xa > 0).double() if c.act == G.RELU else xa * (1 - xa))
    close(dX, want, tol, tol, c.name + " dX")
    if c.name in _PAIRED:
        _kept[c.name] = dX.clone()


def run_wgrad(c):
    from dlrm_amd import ops
    gen = seeded(c)
    Ks = c.K_store or c.K
    dY, X = randn(gen, c.M, c.N), randn(gen, c.M, c.K)
    X[:, Ks:] = 0                                   # the header's contract for a narrower dW: the padding columns of X are zeros
    dyb, xb = in_buf(c, "dy", dY), in_buf(c, "x", X)
    prior_w = randn(gen, c.N, Ks) if c.accumulate else None
    prior_b = randn(gen, c.N) if c.accumulate else None
    wsz = G.workspace_bytes(c)
    ws = ops._scratch("wgrad", wsz, dev()) if c.ws else None

    def once():
        dwb = out_buf(c, "dw", prior_w)
        dball, dbv = vec_buf(c, "dbias", n=c.N, fill=SENT) if c.dbias else (None, None)
        if c.dbias:
            dbv.copy_(prior_b) if c.accumulate else dbv.fill_(float("nan"))
        addr = {"dy": dyb.view.data_ptr(), "x": xb.view.data_ptr(), "dw": dwb.view.data_ptr(), "dbias": dbv.data_ptr() if c.dbias else None,
                "ws": ws.data_ptr() if ws is not None else None, "ws_bytes": ws.numel() if ws is not None else 0}
        check_route(c, addr)
        ops.linear_bwd_weight(dyb.view, xb.view, dwb.view, dbv, accumulate=c.accumulate, use_workspace=c.ws, arith=c.arith)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(dwb.view).any()), "NaN left inside dW"
        assert dwb.outside_is(SENT), "the weight gradient wrote outside dW[N, K_store]"
        if c.dbias:
            assert not bool(torch.isnan(dbv).any()), "NaN left inside dbias"
            chk = dball.clone()
            chk[4: 4 + c.N] = SENT
            assert bool(torch.all(chk == SENT)), "the bias gradient wrote outside dbias[N]"
        return dwb.view, dbv

    dW, db = once()
    work = c.M * c.N * c.K
    if c.arith == "bf16":
        want = product64(rb(dY).t().contiguous(), rb(X).t().contiguous(), work)[:, :Ks]
        rtol, atol, batol = 1e-4, 1e-4 * float(np.sqrt(c.M)), 1e-3
    else:
        want = product64(dY.t().contiguous(), X.t().contiguous(), work)[:, :Ks]
        rtol, atol, batol = 1e-4, 1e-5 * max(1.0, float(want.abs().max())), None
    wantb = dY.double().sum(0)
    if batol is None:
        batol = 1e-4 * max(1.0, float(wantb.abs().max()))
    if c.accumulate:
        want, wantb = want + prior_w.double(), wantb + prior_b.double()
    close(dW, want, rtol, atol, c.name + " dW")
    if c.dbias:
        close(db, wantb, 1e-4, batol, c.name + " dbias")
    if G.EXPECT[c.name][11] or G.EXPECT[c.name][0] in (2, 3):          # slabs summed in a fixed order (and gemv / smallk): deterministic
        dW2, db2 = once()
        assert torch.equal(dW, dW2), "a workspace weight gradient differs between two runs"
        assert not c.dbias or torch.equal(db, db2)


_RUN = {FWD: run_fwd, DGRAD: run_dgrad, WGRAD: run_wgrad}


def _cases(entry):
    cs = [c for c in G.CASES if c.entry == entry]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


@_cases(FWD)
def test_linear_fwd_routes(case):
    run_fwd(case)


@_cases(DGRAD)
def test_linear_bwd_data_routes(case):
    run_dgrad(case)


@_cases(WGRAD)
def test_linear_bwd_weight_routes(case):
    run_wgrad(case)


@pytest.mark.parametrize("a,b", G.EQUIVALENT, ids=["%s=%s" % p for p in G.EQUIVALENT])
def test_equivalent_routes_agree_bit_for_bit(a, b):
    """the straight-line epilogues against the general one (forward: a bias 4 bytes off a 16-byte boundary is all that separates them),
    the sign-bit mask against the fp32 mask (data gradient): same products, same order — identical bits"""
    for n in (a, b):
        if n not in _kept:
            _RUN[G.BY_NAME[n].entry](G.BY_NAME[n])
    assert torch.equal(_kept[a], _kept[b])


@pytest.mark.parametrize("K", [32, 160], ids=["nk1", "nk5"])
@pytest.mark.parametrize("M,N", [(130, 132), (8100, 2044)], ids=["tm2", "tm4"])
def test_gemm_bf16_fp32_shaped_kernel(M, N, K):
    """The two ARITH = 3 instantiations of gemm3_kernel (bf16 operands as stored), which only dlrm_gemm_bf16 launches and only where the
    bf16-shaped kernel of csrc/gemm_bf16.hip declines: here through a bias 4 bytes off a 16-byte boundary (and, at 130 x 132, M < 256).
    128-row tiles at 130 x 132, 256-row tiles at 8100 x 2044 (32 x 16 = 512 workgroups: the `big` rule of dlrm_gemm_bf16, 384 < wg <= 512);
    nk counts 16-word k-tiles of bf16 PAIRS.  Bit-identical to dlrm_linear_fwd(arith = bf16) on the fp32 operands (include/dlrm_hip.h), and
    within the bars of test_linear_bf16_arithmetic of the float64 product of the rounded operands.

    WHAT THIS TEST CANNOT DO: dlrm_gemm_bf16 has no route query, so nothing names the kernel that ran.  That the bf16-shaped kernel
    declines IS pinned on the device — dlrm_gemm_bf16_cross asks the same dlrm_gemm_bf16_phased with the same (M, N, K, pitches, bias) and
    refuses when it declines.  The 128- / 256-row choice behind it is only RESTATED here (`big` of dlrm_gemm_bf16 in csrc/gemm.hip: M >= 256
    and 384 < wg256 <= 512): whoever moves that rule must move the shapes of this test and the reasons in gemm_route_cases.VIA_GEMM_BF16 —
    the test would keep passing on the other tile height."""
    from dlrm_amd import ops
    wg256 = ((M + 255) // 256) * ((N + 127) // 128)
    assert (M >= 256 and 384 < wg256 <= 512) == (M == 8100) and K % 32 == 0 and N % 4 == 0
    g = torch.Generator(device=dev())
    g.manual_seed(M + N + K)
    X, W, b = randn(g, M, K), randn(g, N, K) / float(np.sqrt(K)), randn(g, N)
    ball = torch.empty(N + 1, device=dev())
    bun = ball[1:]
    bun.copy_(b)
    assert bun.data_ptr() % 16 == 4
    Cf = torch.full((M, N), float("nan"), device=dev())
    bits = Bits(M, N)
    A16, B16 = ops.cast_bf16(X, K), ops.cast_bf16(W, K)
    x0 = torch.zeros((M, N), device=dev())
    assert ops.gemm_bf16_cross(A16, B16, bun, x0, x0, want16=False) is None, "the bf16-shaped kernel takes this call: another kernel is under test"
    ops.gemm_bf16(A16, B16, bun, G.RELU, Cf, None, relu_bits_out=bits.view)
    Y = torch.empty((M, N), device=dev())
    ops.linear_fwd(X, W, bun, G.RELU, Y, "bf16")
    torch.cuda.synchronize()
    assert torch.equal(Cf, Y)
    assert torch.equal(bits.decode(), Cf > 0) and bits.guards_intact()
    want = torch.relu(rb(X).double() @ rb(W).double().t() + b.double())
    close(Cf, want, 2e-5, 2e-5, "dlrm_gemm_bf16 on the fp32-shaped kernel")
