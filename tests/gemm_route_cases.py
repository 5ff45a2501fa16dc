"""The case table of the MLP GEMM dispatch (csrc/gemm.hip gemm_route): one row per kernel variant and edge that `dlrm_linear_fwd`,
`dlrm_linear_bwd_data` and `dlrm_linear_bwd_weight` can select, each with the route the library must report for it.

A plain module, shared by tests/test_gemm_routes_host.py (pinning, completeness, boundary sweep: CPU only, fake addresses) and
tests/test_gpu_gemm_routes.py (the same rows run on the device against the float64 oracle).  THE RULE: every gemm3_kernel /
gemm_f32_kernel instantiation compiled into the library is selected by at least one row here, or is listed in UNREACHABLE / VIA_GEMM_BF16
with its reason.  A change of a tile rule therefore has to edit the route tuple written in each row it moves, and a new instantiation needs a row or a reason.

Shapes are the layer's: batch M, outputs N, inputs K (forward Y[M,N] = X[M,K] W[N,K]^T; data gradient dX[M,K] = dY[M,N] W; weight gradient
dW[N,K] = dY^T X, the batch is the reduction).  nk = 16-wide k-tiles per k-slice; the ring of the 128-row fp32 tiles has 2 stages, every
other variant 3.  Reduction lengths 16 (nk = 1, fewer k-tiles than stages) and 80 (nk = 5, more than the ring and no multiple of it) are
used wherever the variant loops over k; the weight gradient's slices are multiples of 32 rows, so there nk = 1 and the odd counts occur in
the LAST slice (M = slices * kchunk + 16 — 7696 = 15 * 512 + 16 for the 256-row tiles — or 4080 = 31 * 128 + 7 * 16 = 7 * 512 + 31 * 16).
"""
from typing import NamedTuple, Optional

FWD, DGRAD, WGRAD = "fwd", "dgrad", "wgrad"
NONE, RELU, SIGMOID = 0, 1, 2


class Case(NamedTuple):
    name: str
    entry: str
    M: int
    N: int
    K: int
    act: int = NONE             # forward: the activation; data gradient: xact_kind of the mask
    arith: str = "f32"
    mask: str = "none"          # forward: "bits" = relu_bits requested; data gradient: "none" | "fp32" | "bits" (Xact AND its sign bits)
    off: tuple = ()             # ((operand, bytes past a 16-byte boundary), ...); operands not named start on a boundary
    ld: tuple = ()              # ((operand, leading dimension), ...); default pitch: columns rounded up to 4, plus 4 (padding to poison)
    bias: bool = True           # forward: a bias vector is passed
    ws: bool = True             # weight gradient: the queried workspace is passed (False: the atomic-accumulation variant)
    accumulate: bool = False
    K_store: Optional[int] = None      # weight gradient: dW is [N, K_store]; X's columns K_store..K-1 are ZERO (the header requires it)
    dbias: bool = True
    # the route the library must report: (path, TM, TN, FRAG, EPI, NST, ARITH, SCHED, splits, kchunk, bits, workspace, atomic),
    # include/dlrm_hip.h DLRM_ROUTE_*; () in the cases the sweeps build
    expect: tuple = ()


# operands of each entry point: name -> (rows, columns) as functions of the case
def operands(c: Case):
    if c.entry == FWD:
        return {"x": (c.M, c.K), "w": (c.N, c.K), "bias": (1, c.N), "y": (c.M, c.N)}
    if c.entry == DGRAD:
        return {"dy": (c.M, c.N), "w": (c.N, c.K), "xact": (c.M, c.K), "dx": (c.M, c.K)}
    return {"dy": (c.M, c.N), "x": (c.M, c.K), "dw": (c.N, c.K_store or c.K), "dbias": (1, c.N)}


def ld_of(c: Case, op: str) -> int:
    d = dict(c.ld)
    if op in d:
        return d[op]
    cols = operands(c)[op][1]
    return ((cols + 3) & ~3) + 4


def off_of(c: Case, op: str) -> int:
    return dict(c.off).get(op, 0)


def fake_addresses(c: Case):
    """addresses for a query without a GPU: the queries look at NULL-ness and alignment only"""
    a = {op: 0x10000000 * (i + 1) + off_of(c, op) for i, op in enumerate(operands(c))}
    a["bits"] = 0x70000000
    a["ws"] = 0x78000000 + off_of(c, "ws")
    return a


def workspace_bytes(c: Case) -> int:
    from dlrm_amd import _lib
    return int(_lib.load().dlrm_linear_bwd_weight_workspace_bytes(c.M, c.N, c.K))


def query(c: Case, addr=None):
    """the library's route for this case; `addr` maps operand names to device addresses (default: fake ones, no GPU needed)"""
    from dlrm_amd import ops
    a = addr or fake_addresses(c)
    if c.entry == FWD:
        return ops.linear_fwd_route(c.M, c.N, c.K, a["x"], ld_of(c, "x"), a["w"], ld_of(c, "w"), a["bias"] if c.bias else None, c.act,
                                    a["y"], ld_of(c, "y"), a["bits"] if c.mask == "bits" else None, c.arith)
    if c.entry == DGRAD:
        masked = c.mask != "none"
        return ops.linear_bwd_data_route(c.M, c.N, c.K, a["dy"], ld_of(c, "dy"), a["w"], ld_of(c, "w"), a["xact"] if masked else None,
                                         ld_of(c, "xact"), c.act if masked else NONE, a["bits"] if c.mask == "bits" else None,
                                         a["dx"], ld_of(c, "dx"), c.arith)
    return ops.linear_bwd_weight_route(c.M, c.N, c.K, c.K_store or c.K, a["dy"], ld_of(c, "dy"), a["x"], ld_of(c, "x"), a["dw"],
                                       ld_of(c, "dw"), a["dbias"] if c.dbias else None, c.accumulate, a["ws"] if c.ws else None,
                                       a.get("ws_bytes", workspace_bytes(c)) if c.ws else 0, c.arith)


FORM = {FWD: (1, 1), DGRAD: (1, 0), WGRAD: (0, 0)}       # (A_KC, B_KC) of gemm3_kernel / gemm_f32_kernel per entry point


def kernel_name(entry: str, route) -> Optional[str]:
    """the mangled-name stem of the instantiation a route launches (None: gemv.hip / smallk.hip, not a GEMM kernel)"""
    a, b = FORM[entry]
    if route.path == 0:
        return "gemm_f32_kernelILb%dELb%dE" % (a, b)
    if route.path != 1:
        return None
    rowsum = int(entry == WGRAD)
    return "gemm3_kernelILb%dELb%dELi%dELi%dELb%dELi%dELi%dELi%dELi%dELi%dE" % (
        a, b, route.tm, route.arith, rowsum, route.frag, route.tn, route.sched, route.nst, route.epi)


def _k(name, expect, entry, M, N, K, **kw):
    """a table row: its name, the route it must take, the call"""
    for f in ("off", "ld"):
        if f in kw:
            kw[f] = tuple(sorted(kw[f].items()))
    assert len(expect) == 13
    return Case(name, entry, M, N, K, expect=expect, **kw)


B4 = {"bias": 4}
CASES = [
    # ------------------------------------------------------------------------------------------------ forward
    # 64 x 64 tiles ("tiny": fewer than 192 workgroups even at 64 x 128); ragged 70 = 64 + 6, 68 = 64 + 4
    _k("fwd_tiny_nk1_bits", (1,1,1,0,0,3,0,0,1,32,0,0,0), FWD, 70, 68, 16, act=RELU, mask="bits"),          # sign bits from the stand-alone kernel
    _k("fwd_tiny_nk5", (1,1,1,0,0,3,0,0,1,96,0,0,0), FWD, 70, 68, 80),
    # 64 x 128 tiles ("small": 96 workgroups at 128 x 128, 192 at 64 x 128); 1500 = 23 * 64 + 28, 1020 = 7 * 128 + 124
    _k("fwd_small_nk1_bits", (1,1,2,0,0,3,0,0,1,32,1,0,0), FWD, 1500, 1020, 16, act=RELU, mask="bits"),
    _k("fwd_small_nk5_sigmoid", (1,1,2,0,0,3,0,0,1,96,0,0,0), FWD, 1500, 1020, 80, act=SIGMOID),
    # 128 x 128 tiles, two-stage ring; 1990 = 15 * 128 + 70: exactly 128 workgroups
    _k("fwd_tm2_epi2_nk1", (1,2,2,0,2,2,0,0,1,32,1,0,0), FWD, 1990, 1020, 16, act=RELU, mask="bits"),
    _k("fwd_tm2_epi2_nk5", (1,2,2,0,2,2,0,0,1,96,1,0,0), FWD, 1990, 1020, 80, act=RELU, mask="bits"),
    _k("fwd_tm2_epi1_nk1", (1,2,2,0,1,2,0,0,1,32,0,0,0), FWD, 1990, 1020, 16),
    _k("fwd_tm2_epi1_nk5", (1,2,2,0,1,2,0,0,1,96,0,0,0), FWD, 1990, 1020, 80),
    _k("fwd_tm2_epi0_sigmoid_nk5", (1,2,2,0,0,2,0,0,1,96,0,0,0), FWD, 1990, 1020, 80, act=SIGMOID),
    _k("fwd_tm2_epi0_bias_off_relu_nk1", (1,2,2,0,0,2,0,0,1,32,1,0,0), FWD, 1990, 1020, 16, act=RELU, mask="bits", off=B4),      # pairs with fwd_tm2_epi2_nk1
    _k("fwd_tm2_epi0_bias_off_relu_nk5", (1,2,2,0,0,2,0,0,1,96,1,0,0), FWD, 1990, 1020, 80, act=RELU, mask="bits", off=B4),      # pairs with fwd_tm2_epi2_nk5
    _k("fwd_tm2_epi0_bias_off_none_nk5", (1,2,2,0,0,2,0,0,1,96,0,0,0), FWD, 1990, 1020, 80, off=B4),                             # pairs with fwd_tm2_epi1_nk5
    _k("fwd_tm2_epi0_n_mod4", (1,2,2,0,0,2,0,0,1,96,1,0,0), FWD, 1990, 1018, 80, act=RELU, mask="bits"),
    _k("fwd_tm2_epi1_no_bias", (1,2,2,0,1,2,0,0,1,96,0,0,0), FWD, 1990, 1020, 80, bias=False),
    # bf16x6 / bf16 MFMA: 128-row tiles at any size (130 = 128 + 2, 132 = 128 + 4), 256-row tiles at 32 x 16 = 512 workgroups
    _k("fwd_bf16x6_tm2_nk1", (1,2,2,0,0,3,1,0,1,32,1,0,0), FWD, 130, 132, 16, act=RELU, mask="bits", arith="bf16x6"),
    _k("fwd_bf16x6_tm2_nk5", (1,2,2,0,0,3,1,0,1,96,0,0,0), FWD, 130, 132, 80, arith="bf16x6"),
    _k("fwd_bf16x6_tm4_nk1", (1,4,2,0,0,3,1,0,1,32,1,0,0), FWD, 8100, 2044, 16, act=RELU, mask="bits", arith="bf16x6"),
    _k("fwd_bf16x6_tm4_nk5", (1,4,2,0,0,3,1,0,1,96,0,0,0), FWD, 8100, 2044, 80, act=SIGMOID, arith="bf16x6"),
    _k("fwd_bf16_tm2_nk1", (1,2,2,0,0,3,2,0,1,32,0,0,0), FWD, 130, 132, 16, arith="bf16"),
    _k("fwd_bf16_tm2_nk5", (1,2,2,0,0,3,2,0,1,96,1,0,0), FWD, 130, 132, 80, act=RELU, mask="bits", arith="bf16"),
    _k("fwd_bf16_tm4_nk1", (1,4,2,0,0,3,2,0,1,32,0,0,0), FWD, 8100, 2044, 16, arith="bf16"),
    _k("fwd_bf16_tm4_nk5", (1,4,2,0,0,3,2,0,1,96,1,0,0), FWD, 8100, 2044, 80, act=RELU, mask="bits", arith="bf16"),
    # N = 1: gemv.hip inside gemv_ok (K % 4 == 0, K <= 1024, aligned rows), the GEMM kernels just outside
    _k("fwd_gemv_k1024", (2,0,0,0,0,0,0,0,1,0,0,0,0), FWD, 300, 1, 1024, act=SIGMOID),
    _k("fwd_gemv_bits", (2,0,0,0,0,0,0,0,1,0,0,0,0), FWD, 300, 1, 256, act=RELU, mask="bits"),
    _k("fwd_n1_k1040_tiny", (1,1,1,0,0,3,0,0,1,1056,0,0,0), FWD, 300, 1, 1040, act=SIGMOID),                  # K > 1024, K % 16 == 0: the 64 x 64 tiles, nk = 65
    _k("fwd_n1_k1028_fallback", (0,0,0,0,0,0,0,0,1,1056,0,0,0), FWD, 300, 1, 1028, act=SIGMOID),              # K > 1024, K % 16 != 0
    _k("fwd_gemv_bias_off", (2,0,0,0,0,0,0,0,1,0,0,0,0), FWD, 300, 1, 256, act=SIGMOID, off={"bias": 4}),  # (the bias alignment is no gemv precondition)
    _k("fwd_n1_w_off_fallback", (0,0,0,0,0,0,0,0,1,256,0,0,0), FWD, 300, 1, 256, act=SIGMOID, off={"w": 4}),
    # the any-shape kernel, one precondition at a time
    _k("fwd_fallback_k_mod16", (0,0,0,0,0,0,0,0,1,32,0,0,0), FWD, 130, 132, 20, act=RELU, mask="bits"),
    _k("fwd_fallback_ld_mod4", (0,0,0,0,0,0,0,0,1,32,0,0,0), FWD, 130, 132, 32, act=RELU, ld={"x": 35}),
    _k("fwd_fallback_ptr_off", (0,0,0,0,0,0,0,0,1,32,0,0,0), FWD, 130, 132, 32, off={"w": 4}),
    # ------------------------------------------------------------------------------------------------ data gradient (output [M, K], reduce N)
    _k("dgrad_tiny_nk1", (1,1,1,1,0,3,0,0,1,32,0,0,0), DGRAD, 70, 16, 68),
    _k("dgrad_tiny_nk5_fp32", (1,1,1,1,0,3,0,0,1,96,0,0,0), DGRAD, 70, 80, 68, act=RELU, mask="fp32"),
    _k("dgrad_tiny_nk5_bits", (1,1,1,1,0,3,0,0,1,96,0,0,0), DGRAD, 70, 80, 68, act=RELU, mask="bits"),      # the 64 x 64 tiles read no bits: the fp32 mask, same kernel
    _k("dgrad_small_nk1_fp32", (1,1,2,1,0,3,0,0,1,32,0,0,0), DGRAD, 1500, 16, 1020, act=RELU, mask="fp32"),
    _k("dgrad_small_nk1_bits", (1,1,2,1,0,3,0,0,1,32,1,0,0), DGRAD, 1500, 16, 1020, act=RELU, mask="bits"),
    _k("dgrad_small_nk5_fp32", (1,1,2,1,0,3,0,0,1,96,0,0,0), DGRAD, 1500, 80, 1020, act=RELU, mask="fp32"),
    _k("dgrad_small_nk5_bits", (1,1,2,1,0,3,0,0,1,96,1,0,0), DGRAD, 1500, 80, 1020, act=RELU, mask="bits"),
    _k("dgrad_tm2_epi1_nk1", (1,2,2,1,1,2,0,0,1,32,0,0,0), DGRAD, 1990, 16, 1020),
    _k("dgrad_tm2_epi1_nk5_bits", (1,2,2,1,1,2,0,0,1,96,1,0,0), DGRAD, 1990, 80, 1020, act=RELU, mask="bits"),
    _k("dgrad_tm2_epi0_nk5_fp32", (1,2,2,1,0,2,0,0,1,96,0,0,0), DGRAD, 1990, 80, 1020, act=RELU, mask="fp32"),
    _k("dgrad_tm2_epi1_nk1_bits", (1,2,2,1,1,2,0,0,1,32,1,0,0), DGRAD, 1990, 16, 1020, act=RELU, mask="bits"),
    _k("dgrad_tm2_epi0_nk1_fp32", (1,2,2,1,0,2,0,0,1,32,0,0,0), DGRAD, 1990, 16, 1020, act=RELU, mask="fp32"),
    _k("dgrad_tm2_epi0_sigmoid", (1,2,2,1,0,2,0,0,1,96,0,0,0), DGRAD, 1990, 80, 1020, act=SIGMOID, mask="fp32"),
    _k("dgrad_tm2_epi0_k_mod4", (1,2,2,1,0,2,0,0,1,96,0,0,0), DGRAD, 1990, 80, 1018),
    _k("dgrad_bf16x6_tm2_nk1", (1,2,2,0,0,3,1,0,1,32,0,0,0), DGRAD, 130, 16, 132, arith="bf16x6"),
    _k("dgrad_bf16x6_tm2_nk5_fp32", (1,2,2,0,0,3,1,0,1,96,0,0,0), DGRAD, 130, 80, 132, act=RELU, mask="fp32", arith="bf16x6"),
    _k("dgrad_bf16x6_tm2_nk5_bits", (1,2,2,0,0,3,1,0,1,96,1,0,0), DGRAD, 130, 80, 132, act=RELU, mask="bits", arith="bf16x6"),
    _k("dgrad_bf16x6_tm4_nk1_bits", (1,4,2,0,0,3,1,0,1,32,1,0,0), DGRAD, 8100, 16, 2044, act=RELU, mask="bits", arith="bf16x6"),
    _k("dgrad_bf16x6_tm4_nk5", (1,4,2,0,0,3,1,0,1,96,0,0,0), DGRAD, 8100, 80, 2044, arith="bf16x6"),
    _k("dgrad_bf16_tm2_nk1_bits", (1,2,2,0,0,3,2,0,1,32,1,0,0), DGRAD, 130, 16, 132, act=RELU, mask="bits", arith="bf16"),
    _k("dgrad_bf16_tm2_nk5", (1,2,2,0,0,3,2,0,1,96,0,0,0), DGRAD, 130, 80, 132, arith="bf16"),
    _k("dgrad_bf16_tm4_nk1", (1,4,2,0,0,3,2,0,1,32,0,0,0), DGRAD, 8100, 16, 2044, arith="bf16"),
    _k("dgrad_bf16_tm4_nk5_fp32", (1,4,2,0,0,3,2,0,1,96,0,0,0), DGRAD, 8100, 80, 2044, act=RELU, mask="fp32", arith="bf16"),
    _k("dgrad_bf16_tm4_nk5_bits", (1,4,2,0,0,3,2,0,1,96,1,0,0), DGRAD, 8100, 80, 2044, act=RELU, mask="bits", arith="bf16"),
    _k("dgrad_gemv_k1024", (2,0,0,0,0,0,0,0,1,0,0,0,0), DGRAD, 300, 1, 1024, act=RELU, mask="fp32"),
    _k("dgrad_n1_k1028_fallback", (0,0,0,0,0,0,0,0,1,32,0,0,0), DGRAD, 300, 1, 1028, act=RELU, mask="fp32"),
    _k("dgrad_n1_xact_off_fallback", (0,0,0,0,0,0,0,0,1,32,0,0,0), DGRAD, 300, 1, 256, act=RELU, mask="fp32", off={"xact": 4}),
    _k("dgrad_fallback_n_mod16", (0,0,0,0,0,0,0,0,1,32,0,0,0), DGRAD, 130, 20, 132, act=RELU, mask="bits"),
    _k("dgrad_fallback_ld_mod4", (0,0,0,0,0,0,0,0,1,32,0,0,0), DGRAD, 130, 32, 132, act=RELU, mask="fp32", ld={"w": 137}),
    _k("dgrad_fallback_ptr_off", (0,0,0,0,0,0,0,0,1,32,0,0,0), DGRAD, 130, 32, 132, off={"dy": 4}),
    # ------------------------------------------------------------------------------------------------ weight gradient (output [N, K], reduce M)
    # 64 x 64 tiles
    _k("wgrad_tiny_one_slice_nk1", (1,1,1,1,0,3,0,0,1,32,0,0,0), WGRAD, 16, 68, 68),
    _k("wgrad_tiny_ws_last_nk1", (1,1,1,1,0,3,0,0,5,128,0,1,0), WGRAD, 528, 68, 68),                          # 5 slices of 128 rows (the last 16): 20 workgroups, not a multiple of 8
    _k("wgrad_tiny_atomic_last_nk1", (1,1,1,1,0,3,0,0,5,128,0,0,1), WGRAD, 528, 68, 68, ws=False),
    _k("wgrad_tiny_ws_8wg", (1,1,1,1,0,3,0,0,2,96,0,1,0), WGRAD, 176, 68, 68),                               # 2 slices of 96 / 80 rows (nk 6, 5): 8 workgroups
    _k("wgrad_tiny_kstore", (1,1,1,1,0,3,0,0,5,128,0,1,0), WGRAD, 528, 68, 68, K_store=65),
    # 64 x 128 tiles
    _k("wgrad_small_one_slice_nk1", (1,1,2,1,0,3,0,0,1,32,0,0,0), WGRAD, 16, 4092, 260),
    _k("wgrad_small_ws_last_nk1", (1,1,2,1,0,3,0,0,5,128,0,1,0), WGRAD, 528, 516, 516),                       # 225 workgroups
    _k("wgrad_small_atomic_last_nk1", (1,1,2,1,0,3,0,0,5,128,0,0,1), WGRAD, 528, 1500, 132, ws=False),        # 240 workgroups
    _k("wgrad_small_ws_last_nk7", (1,1,2,1,0,3,0,0,32,128,0,1,0), WGRAD, 4080, 68, 260),                       # 32 slices of 128 rows, the last 112
    # 128 x 128 tiles, two-stage ring
    _k("wgrad_tm2_epi1_one_slice_nk1", (1,2,2,1,1,2,0,1,1,32,0,0,0), WGRAD, 16, 1020, 2040),                 # stores straight into dW
    _k("wgrad_tm2_epi0_one_slice_dw_off", (1,2,2,1,0,2,0,1,1,32,0,0,0), WGRAD, 16, 1020, 2040, off={"dw": 4}),
    _k("wgrad_tm2_epi0_one_slice_accumulate", (1,2,2,1,0,2,0,1,1,32,0,0,1), WGRAD, 16, 1020, 2040, accumulate=True),      # one slice, atomics because it accumulates
    _k("wgrad_tm2_ws_last_nk1", (1,2,2,1,1,2,0,1,9,128,0,1,0), WGRAD, 1040, 260, 516),                        # 9 slices: 135 workgroups
    _k("wgrad_tm2_atomic_last_nk1", (1,2,2,1,0,2,0,1,9,128,0,0,1), WGRAD, 1040, 260, 516, ws=False),
    _k("wgrad_tm2_ws_last_nk7", (1,2,2,1,1,2,0,1,32,128,0,1,0), WGRAD, 4080, 132, 132),                        # 32 slices: 128 workgroups
    _k("wgrad_tm2_atomic_last_nk7", (1,2,2,1,0,2,0,1,32,128,0,0,1), WGRAD, 4080, 132, 132, ws=False),
    _k("wgrad_tm2_ws_accumulate", (1,2,2,1,1,2,0,1,9,128,0,1,0), WGRAD, 1040, 260, 516, accumulate=True),
    _k("wgrad_tm2_atomic_accumulate", (1,2,2,1,0,2,0,1,9,128,0,0,1), WGRAD, 1040, 260, 516, ws=False, accumulate=True),
    _k("wgrad_tm2_kstore", (1,2,2,1,1,2,0,1,9,128,0,1,0), WGRAD, 1040, 260, 516, K_store=513),
    _k("wgrad_tm2_ws_no_dbias", (1,2,2,1,1,2,0,1,9,128,0,1,0), WGRAD, 1040, 260, 516, dbias=False),
    # 256 x 128 tiles (fp32: split-k only): 8 slices of 512 rows, the last 496 (nk 32, 31); 8 x 8 x 8 = 512 workgroups
    _k("wgrad_tm4_ws", (1,4,2,1,1,3,0,1,8,512,0,1,0), WGRAD, 4080, 2040, 1020),
    _k("wgrad_tm4_atomic", (1,4,2,1,0,3,0,1,8,512,0,0,1), WGRAD, 4080, 2040, 1020, ws=False),
    # ... and 16 slices of 512 rows, the last of 16 (nk = 1 behind slices of nk = 32): 4 x 8 x 16 = 512 workgroups
    _k("wgrad_tm4_ws_last_nk1", (1,4,2,1,1,3,0,1,16,512,0,1,0), WGRAD, 7696, 1020, 1020),
    _k("wgrad_tm4_atomic_last_nk1", (1,4,2,1,0,3,0,1,16,512,0,0,1), WGRAD, 7696, 1020, 1020, ws=False),
    # bf16x6 / bf16 MFMA
    _k("wgrad_bf16x6_tm2_one_slice_nk1", (1,2,2,0,0,3,1,0,1,32,0,0,0), WGRAD, 16, 132, 260, arith="bf16x6"),
    _k("wgrad_bf16x6_tm2_ws_last_nk1", (1,2,2,0,0,3,1,0,5,128,0,1,0), WGRAD, 528, 132, 132, arith="bf16x6"),
    _k("wgrad_bf16x6_tm2_atomic", (1,2,2,0,0,3,1,0,2,96,0,0,1), WGRAD, 176, 132, 132, ws=False, arith="bf16x6"),
    _k("wgrad_bf16x6_tm4_atomic", (1,4,2,0,0,3,1,0,8,512,0,0,1), WGRAD, 4080, 2040, 1020, ws=False, arith="bf16x6"),
    _k("wgrad_bf16x6_tm4_one_slice_nk1", (1,4,2,0,0,3,1,0,1,32,0,0,0), WGRAD, 16, 4092, 4092, arith="bf16x6"),
    _k("wgrad_bf16x6_tm4_ws", (1,4,2,0,0,3,1,0,8,512,0,1,0), WGRAD, 4080, 2040, 1020, arith="bf16x6"),
    _k("wgrad_bf16_tm2_one_slice_nk1", (1,2,2,0,0,3,2,0,1,32,0,0,0), WGRAD, 16, 132, 260, arith="bf16"),
    _k("wgrad_bf16_tm2_ws_last_nk1", (1,2,2,0,0,3,2,0,5,128,0,1,0), WGRAD, 528, 132, 132, arith="bf16"),
    _k("wgrad_bf16_tm2_atomic", (1,2,2,0,0,3,2,0,2,96,0,0,1), WGRAD, 176, 132, 132, ws=False, arith="bf16"),
    _k("wgrad_bf16_tm4_ws", (1,4,2,0,0,3,2,0,8,512,0,1,0), WGRAD, 4080, 2040, 1020, arith="bf16"),
    _k("wgrad_bf16_tm4_one_slice_nk1", (1,4,2,0,0,3,2,0,1,32,0,0,0), WGRAD, 16, 4092, 4092, arith="bf16"),
    _k("wgrad_bf16_tm4_atomic", (1,4,2,0,0,3,2,0,8,512,0,0,1), WGRAD, 4080, 2040, 1020, ws=False, arith="bf16"),
    # N = 1 (gemv.hip needs its workspace) and K <= 16 at M >= 4096 (smallk.hip)
    _k("wgrad_gemv_k1024", (2,0,0,0,0,0,0,0,1,0,0,1,0), WGRAD, 300, 1, 1024),
    _k("wgrad_n1_no_ws_fallback", (0,0,0,0,0,0,0,0,3,128,0,0,1), WGRAD, 300, 1, 1024, ws=False),             # 300 % 16 != 0: the any-shape kernel
    _k("wgrad_n1_k1028", (1,1,1,1,0,3,0,0,3,128,0,1,0), WGRAD, 304, 1, 1028),                                # K % 4 == 0 but > 1024: the 64 x 64 tiles
    _k("wgrad_smallk_m4096", (3,0,0,0,0,0,0,0,1,0,0,1,0), WGRAD, 4096, 64, 16),
    _k("wgrad_smallk_kstore", (3,0,0,0,0,0,0,0,1,0,0,1,0), WGRAD, 4096, 64, 16, K_store=13),
    _k("wgrad_k16_m4095_fallback", (0,0,0,0,0,0,0,0,32,128,0,1,0), WGRAD, 4095, 64, 16),                      # below 4096 rows — and 4095 % 16 != 0
    _k("wgrad_k16_m4080_tiny", (1,1,1,1,0,3,0,0,32,128,0,1,0), WGRAD, 4080, 64, 16),                          # below 4096 rows: the 64 x 64 tiles
    _k("wgrad_k16_m4096_no_ws_tiny", (1,1,1,1,0,3,0,0,32,128,0,0,1), WGRAD, 4096, 64, 16, ws=False),
    # the any-shape kernel, one precondition at a time
    _k("wgrad_fallback_m_mod16", (0,0,0,0,0,0,0,0,8,128,0,1,0), WGRAD, 1000, 132, 132),
    _k("wgrad_fallback_ld_mod4", (0,0,0,0,0,0,0,0,9,128,0,1,0), WGRAD, 1040, 132, 132, ld={"x": 137}),
    _k("wgrad_fallback_ptr_off", (0,0,0,0,0,0,0,0,9,128,0,0,1), WGRAD, 1040, 132, 132, off={"dy": 4}, ws=False),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# bit-for-bit pairs of the device test: (case, case) computing the same values through different epilogues / mask sources
EQUIVALENT = [
    ("fwd_tm2_epi2_nk1", "fwd_tm2_epi0_bias_off_relu_nk1"), ("fwd_tm2_epi2_nk5", "fwd_tm2_epi0_bias_off_relu_nk5"),
    ("fwd_tm2_epi1_nk5", "fwd_tm2_epi0_bias_off_none_nk5"),
    ("dgrad_tiny_nk5_fp32", "dgrad_tiny_nk5_bits"), ("dgrad_small_nk1_fp32", "dgrad_small_nk1_bits"),
    ("dgrad_small_nk5_fp32", "dgrad_small_nk5_bits"), ("dgrad_tm2_epi0_nk5_fp32", "dgrad_tm2_epi1_nk5_bits"),
    ("dgrad_tm2_epi0_nk1_fp32", "dgrad_tm2_epi1_nk1_bits"),
]

# name -> the pinned route (the table above is the one place a tile-rule change edits)
EXPECT = {c.name: c.expect for c in CASES}

# ---- compiled instantiations no row can select, with the reason; tests/test_gemm_routes_host.py proves each "unreachable" by a sweep
_G3 = "gemm3_kernelILb%dELb%dELi%dELi%dELb%dELi%dELi%dELi%dELi%dELi%dE"
UNREACHABLE = {}
for _e in (1, 2, 0):      # fp32 256-row tiles of the one-slice forms: splits == 1 clears `big` for fp32 (the forward; EPI 0 / 1 / 2)
    UNREACHABLE[_G3 % (1, 1, 4, 0, 0, 0, 2, 0, 3, _e)] = "unreachable in the product build because splits == 1 clears `big` for fp32 (forward)"
for _f in (0, 1):
    for _e in (0, 1):     # ... and of the data gradient, with either fragment layout
        UNREACHABLE[_G3 % (1, 0, 4, 0, 0, _f, 2, 0, 3, _e)] = \
            "unreachable in the product build because splits == 1 clears `big` for fp32 (data gradient)"
for _a, _b, _rs, _sd in ((1, 0, 0, 0), (0, 0, 1, 1)):      # fp32 scalar fragments (FRAG 0) of the two k-strided forms: `frag` folds to 1
    _why = "unreachable in the product build because `frag` folds to 1: fp32 calls of the k-strided forms take the FRAG = 1 kernels"
    UNREACHABLE[_G3 % (_a, _b, 1, 0, _rs, 0, 1, 0, 3, 0)] = _why
    UNREACHABLE[_G3 % (_a, _b, 1, 0, _rs, 0, 2, 0, 3, 0)] = _why
    for _e in (0, 1):
        UNREACHABLE[_G3 % (_a, _b, 2, 0, _rs, 0, 2, _sd, 2, _e)] = _why
        UNREACHABLE.setdefault(_G3 % (_a, _b, 4, 0, _rs, 0, 2, _sd, 3, _e), _why)

# ARITH = 3 (bf16 operands as stored): launched by dlrm_gemm_bf16 only, where the bf16-shaped kernel of gemm_bf16.hip declines
VIA_GEMM_BF16 = {
    _G3 % (1, 1, 2, 3, 0, 0, 2, 0, 3, 0): "reached only through dlrm_gemm_bf16, covered by "
                                          "tests/test_gpu_elementwise.py::test_gemm_bf16_addend_refusals_write_nothing (M = 128) and "
                                          "tests/test_gpu_gemm_routes.py::test_gemm_bf16_fp32_shaped_kernel[tm2]",
    _G3 % (1, 1, 4, 3, 0, 0, 2, 0, 3, 0): "reached only through dlrm_gemm_bf16, covered by "
                                          "tests/test_gpu_gemm_routes.py::test_gemm_bf16_fp32_shaped_kernel[tm4]",
}
