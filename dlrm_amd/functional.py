"""Autograd glue: torch.autograd.Function wrappers around the HIP kernels (dlrm_amd.ops).

The Functions exchange STRIDED VIEWS of shared buffers instead of copies:
  * the bottom tower writes its output straight into slot 0 of the [B, F*D] interaction buffer and
    the embedding kernel into slots 1..T (no torch.cat),
  * interaction backward writes per-input gradient chunks that the embedding update kernel, the
    bottom tower backward and (distributed) the reverse all-to-all consume in place.
Backward runs on the autograd engine's thread: streams/devices are looked up at call time.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence

import weakref

import torch
from torch.autograd import Function

from . import ops
from .ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, _ld


# optional: weight-gradient GEMMs on a side stream, concurrent with the data-gradient chain (env DLRM_OVERLAP_WGRAD=1).
# Measured on MI355X (profiles/r01, g02): 11.83 ms/step with the overlap vs 11.30 ms without — two chip-filling GEMMs
# sharing the CUs thrash each other's L2 panels — so it is OFF by default.
OVERLAP_WGRAD = os.environ.get("DLRM_OVERLAP_WGRAD", "0") == "1"
# ... except for SMALL batches inside a HIP-graph capture: rows at or below this run weight and data gradient concurrently (0 = never)
SMALL_BATCH_OVERLAP = int(os.environ.get("DLRM_SMALL_BATCH_OVERLAP", "8192"))
SMALL_BATCH_BITS = int(os.environ.get("DLRM_SMALL_BATCH_BITS", "8192"))      # no ReLU sign bits at or below this many rows (fp32 towers)
# hidden ReLU layers store 1 sign bit per activation for the next layer's data-gradient epilogue (DLRM_RELU_BITS=0: the
# epilogue re-reads the fp32 activation instead)
RELU_BITS = os.environ.get("DLRM_RELU_BITS", "1") == "1"
# arith "bf16": activations / weights are also kept as bf16 copies and the GEMMs read those (dlrm_gemm_bf16) instead of rounding fp32
# operands inside the k-loop (DLRM_BF16_STORAGE=0: the in-loop rounding of rounds 1-2; results are bit-identical)
BF16_STORAGE = os.environ.get("DLRM_BF16_STORAGE", "1") == "1"
# bf16 storage, LEAN: hidden activations / gradients exist only as bf16 (+ ReLU sign bits) wherever every consumer reads bf16 (MLPFunction)
BF16_LEAN = os.environ.get("DLRM_BF16_LEAN", "1") == "1"
# DCN-v2 (bf16 storage): the elementwise half of a cross layer inside the epilogue of its second product (dlrm_gemm_bf16_cross); 0 = two kernels
CROSS_FUSE = os.environ.get("DLRM_CROSS_FUSE", "1") == "1"      # (1: the forward x_{l+1} is bit-identical to the two kernels, but the backward reads bf16(u) instead of the fp32 u: gradients differ at that rounding — INTEGRATION.md)
# small batches: a whole fp32 tower per launch (csrc/tower.hip) for up to DLRM_TOWER_ROWS rows (0 = never: the per-layer GEMMs) while the
# weight traffic of its 16-row workgroups stays under DLRM_TOWER_L2_MB; see _tower_applies.  Criteo-Kaggle graph: 44 -> 19 kernels per step,
# 0.367 -> 0.357 ms (profiles/round5/kaggle_towers.md)
TOWER_ROWS = int(os.environ.get("DLRM_TOWER_ROWS", "4096"))
TOWER_L2_BYTES = int(os.environ.get("DLRM_TOWER_L2_MB", "384")) << 20
# ... and which half of a tower they take: the BACKWARD launches always (data-gradient chain + grouped weight gradients: 2-3 launches instead
# of 3 per layer), the forward launch only with DLRM_TOWER_FWD=1 — the per-layer forward GEMMs spread every layer over the whole chip and are
# faster than one 128-workgroup tower launch (Criteo-Kaggle graph: 0.358 ms with the tower forward, 0.319 without, 0.362 with no tower kernels)
TOWER_FWD = os.environ.get("DLRM_TOWER_FWD", "0") == "1"
# flag bit of MLPFunction's `arith` argument (see MLPFunction.forward); DLRM_FUSE_ACT_BWD=0 makes DLRM_Net never set it (A/B)
MLP_CONSUMER_APPLIES_LAST_ACT = 0x100
FUSE_ACT_BWD = os.environ.get("DLRM_FUSE_ACT_BWD", "1") == "1"
# bf16 towers: the bf16 copies of ALL weights of a tower (W16 for the forward GEMMs, W^T16 for the data gradients) in one launch at the start of
# the forward pass (dlrm_cast_bf16_multi) instead of one launch per layer and direction; 0 = per-layer casts
MULTI_CAST = os.environ.get("DLRM_BF16_MULTI_CAST", "1") == "1"
# arith "bf16x6": activations / gradients / weights of the GEMM layers travel as three bf16 planes (split once by their producer) and the GEMMs
# are the planes form of the bf16-shaped kernel (dlrm_gemm_bf16x6), wherever its shapes hold (DLRM_BF16X6_PLANES=0: every GEMM splits its fp32
# operands inside its k-loop, the kernels of rounds 1-3; the k-contiguous products are bit-identical either way)
BF16X6_PLANES = os.environ.get("DLRM_BF16X6_PLANES", "1") == "1"
# the N == 1 head of a tower (256 -> 1 + sigmoid): its whole backward in one pass over its input (DLRM_HEAD_FUSED=0: the three calls)
HEAD_FUSED = os.environ.get("DLRM_HEAD_FUSED", "1") == "1"
_side_streams = {}


class _Bf16Store:
    """how MLPFunction keeps the reduced-width copies of arith "bf16": one bf16 matrix per tensor"""
    planes = False
    kround = staticmethod(ops.round_bf16_k)
    cast = staticmethod(ops.cast_bf16)
    cast_t = staticmethod(ops.cast_bf16_transposed)
    cast_multi = staticmethod(ops.cast_bf16_multi)           # several (copy, transposed copy) pairs in one launch
    gemm = staticmethod(ops.gemm_bf16)
    wgrad = staticmethod(ops.linear_bwd_weight_bf16)
    wgrad_ok = staticmethod(ops.linear_bwd_weight_bf16_ok)

    @staticmethod
    def empty(M, N, device):
        return torch.empty((M, N), dtype=torch.bfloat16, device=device)

    @staticmethod
    def fwd_ok(M, N, K):        # (dlrm_gemm_bf16 keeps the fp32-shaped kernel for shapes the bf16-shaped one does not take)
        return True


class _PlaneStore:
    """... and of arith "bf16x6": the three bf16 planes of the fp32 tensor, [3, rows, cols] (ops.split_bf16x3)"""
    planes = True
    kround = staticmethod(ops.round_x6_k)
    cast = staticmethod(ops.split_bf16x3)
    cast_t = staticmethod(ops.split_bf16x3_transposed)
    gemm = staticmethod(ops.gemm_bf16x6)
    wgrad = staticmethod(ops.linear_bwd_weight_bf16x6)

    @staticmethod
    def wgrad_ok(M, N, K, dZ3, X3):
        return ops.linear_bwd_weight_bf16_ok(M, N, K, dZ3[0], X3[0])

    @staticmethod
    def empty(M, N, device):
        return torch.empty((3, M, N), dtype=torch.bfloat16, device=device)

    @staticmethod
    def fwd_ok(M, N, K):        # no other kernel reads planes: exactly the preconditions of dlrm_gemm_bf16x6
        return ops.gemm_bf16x6_ok(M, N, K)


def _side_stream(device) -> "torch.cuda.Stream":
    st = _side_streams.get(device)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[device] = st
    return st


def _wgrad_overlaps(M: int) -> bool:
    """the weight-gradient GEMMs of an M-row backward pass go to the side stream: always with OVERLAP_WGRAD; otherwise for SMALL batches
    — Criteo-Kaggle's 2048 rows — where every GEMM of the step occupies a fraction of the chip, so the independent weight-gradient launch runs
    BESIDE the data-gradient launch for free; the fork / join are events a graph capture records — measured at Criteo-Kaggle shapes: graphed
    step 0.515 -> 0.497 ms; in the EAGER step the two extra event records per layer cost the host more than the overlap saves
    (1.51 -> 1.74 ms), so only a capturing stream forks"""
    return OVERLAP_WGRAD or (0 < SMALL_BATCH_OVERLAP and M <= SMALL_BATCH_OVERLAP and torch.cuda.is_current_stream_capturing())


# A parameter wrapped by ext_dist.FlatDDP carries `p._dlrm_grad_arena = (weakref to the flat fp32 gradient buffer, element offset)`:
# the weight-gradient GEMMs of MLPFunction write such a parameter's gradient straight into the flat buffer that FlatDDP all-reduces
# (no bucket copy in, none out).  The slot lives ON the Parameter object (not in a table keyed by its address): a tower that is
# moved with .to(), re-created, or whose wrapper is discarded can never be redirected into a stale buffer.
ARENA_BUSY = set()      # id(parameter) of slots handed out in the running backward pass whose gradient autograd has not accumulated yet


def set_grad_arena(p: torch.Tensor, flat: Optional[torch.Tensor], offset: int = 0) -> None:
    if flat is None:
        if hasattr(p, "_dlrm_grad_arena"):
            del p._dlrm_grad_arena
        ARENA_BUSY.discard(id(p))
        return
    p._dlrm_grad_arena = (weakref.ref(flat), int(offset))


def _grad_out(p: torch.Tensor) -> torch.Tensor:
    a = getattr(p, "_dlrm_grad_arena", None)
    flat = a[0]() if a is not None else None
    if flat is None:
        return torch.empty_like(p)
    off = a[1]
    if (flat.device != p.device or flat.dtype != p.dtype or off < 0 or off + p.numel() > flat.numel()
            or (flat.data_ptr() + 4 * off) % 16 != 0):
        raise RuntimeError("dlrm_amd: the flat gradient buffer of this parameter does not match it any more (device %s vs %s, "
                           "%d + %d of %d elements); re-wrap the tower in ext_dist.FlatDDP after moving it"
                           % (flat.device, p.device, off, p.numel(), flat.numel()))
    v = flat[off:off + p.numel()].view(p.shape)
    key = id(p)
    # one writer per slot: a second use of the tower in the same backward pass (the pipelined exchange applies the top tower once per
    # chunk) or the gradient of an earlier backward pass still living there (accumulation) get a tensor of their own — autograd sums
    # them and FlatDDP moves the sum into the flat buffer
    if key in ARENA_BUSY or (p.grad is not None and p.grad.data_ptr() == v.data_ptr()):
        return torch.empty_like(p)
    ARENA_BUSY.add(key)
    return v


def _round4(n: int) -> int:
    return (n + 3) & ~3


def alloc2d(M: int, N: int, like: torch.Tensor, zero: bool = False) -> torch.Tensor:
    """[M, N] view of an [M, round_up(N, 4)] buffer: every row starts 16-byte aligned.  A single column stays [M, 1]
    contiguous (the matrix-vector kernels take any pitch, and the loss kernel reads the predictions in place)."""
    ldn = 1 if N == 1 else _round4(N)
    buf = (torch.zeros if zero else torch.empty)((M, ldn), dtype=torch.float32, device=like.device)
    return buf if ldn == N else buf[:, :N]


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dim() == 2 and t.stride(1) == 1) or t.numel() == 0 else t.contiguous()


class OutSlot:
    """A caller-provided destination view handed to a Function without being an autograd input."""

    def __init__(self, view: torch.Tensor):
        self._view = view

    def get(self) -> torch.Tensor:
        return self._view[:]  # fresh tensor object sharing the storage (gets its own grad_fn)


_F32, _BF16, _BF16X6 = (ops.arith_code(a) for a in ("f32", "bf16", "bf16x6"))


def _tower_path_ok(M, in_width, dims, arith, on_gpu) -> bool:
    """the small-batch tower kernels take this MLP: native fp32, a batch of at most TOWER_ROWS rows, widths the kernels hold in LDS, and
    little enough weight traffic — every 16-row workgroup streams ALL weights, (M / 16) x parameters x 4 bytes through L2, which is what
    bounds the path to small batches x small towers (Criteo-Kaggle: 128 x 1.3 MB; the Criteo-Terabyte towers at 2048 rows would move 1.1 GB)"""
    if TOWER_ROWS <= 0 or not on_gpu or arith != _F32:
        return False
    L = len(dims)
    K0 = dims[0][1]
    if M < 1 or M > TOWER_ROWS or in_width not in (K0, _round4(K0)) or L > ops.TOWER_MAX_LAYERS:
        return False
    widths = [in_width] + [N for N, _ in dims]
    if not ops.tower_ok(M, widths):
        return False
    if any(dims[i][1] != (K0 if i == 0 else widths[i]) for i in range(L)):
        return False
    weight_bytes = 4 * sum(widths[i] * widths[i + 1] for i in range(L))
    return ((M + 15) // 16) * weight_bytes <= TOWER_L2_BYTES


def _tower_applies(x, arith, params, L) -> bool:
    return _tower_path_ok(x.size(0), x.size(1), [(params[2 * i].size(0), params[2 * i].size(1)) for i in range(L)], arith, x.is_cuda)


class LayerPlan(NamedTuple):
    """one layer of a TowerPlan: y = act(in . W^T + b), W [N, K] (K of the first layer: the padded width its GEMMs run on)"""
    N: int
    K: int
    act: int
    # forward
    out32: bool = True          # the fp32 output is allocated (and saved for backward)
    fwd16: bool = False         # kernel form: st.gemm on reduced-width operands (else ops.linear_fwd on fp32)
    kb: int = 0                 # ... whose reduction length is padded to this
    out16: bool = False         # the reduced-width output is allocated: the next layer's GEMM reads it as it is
    bits: bool = False          # ReLU sign bits are allocated (a hidden ReLU layer of a tower that keeps bits)
    w16_multi: bool = False     # W16 comes out of the tower's multi-cast launch
    wT16_multi: bool = False    # ... and so does W^T16, for the data gradient
    # backward
    wgrad16: bool = False       # weight gradient from the reduced-width operands as stored; forward keeps its reduced-width input for it
    need_dx: bool = True        # a data gradient is computed (the first layer's only if the tower's input wants one)
    dgrad16: bool = False       # data gradient as a reduced-width GEMM over W^T16 (else ops.linear_bwd_data on fp32)
    dx32: bool = True           # the data gradient is written as fp32
    dx16: bool = False          # ... in reduced width (both may hold)
    mask_act: int = ACT_NONE    # the derivative its epilogue applies: the activation of the layer below
    mask_bits: bool = False     # ... read from that layer's sign bits (the fp32 form also needs its fp32 output; the reduced-width one does not)


class TowerPlan(NamedTuple):
    """every decision MLPFunction makes for one call, forward and backward (_plan_tower); neither pass derives any of them again"""
    layers: tuple
    acts: tuple
    arith: int
    whole_tower: bool           # backward (and with tower_fwd: forward) on the whole-tower kernels of csrc/tower.hip
    tower_fwd: bool
    store: Optional[type]       # None, _Bf16Store or _PlaneStore: how reduced-width copies are kept
    in_width: int               # width of x as it arrives
    pad_x: bool                 # x is copied into a zero-padded buffer Kp wide
    Kp: int                     # the first weight is zero-padded to this width (0: used as it is)
    need_bits: bool
    multi_cast: bool            # all W16 / W^T16 of the tower in one launch
    need_dx: bool               # the tower's input wants a gradient
    head_fused: bool            # backward may try the one-pass N == 1 head
    consumer_act: bool          # MLP_CONSUMER_APPLIES_LAST_ACT


_WIDTH_ERR = "dlrm_amd: MLP input width %d does not match the first layer (%d)"


def _plan_tower(M, in_width, dims, acts, arith, need_grad, need_dx, on_gpu, has_slot=False, slot_aligned=True, consumer_act=False) -> TowerPlan:
    """The storage and kernel plan of one MLPFunction call, from integers and booleans alone (dims: (N_i, K_i) of every weight; slot_aligned:
    the out_slot's rows are 16-byte aligned, ld % 4 == 0).  Allocates nothing; reads the module switches when called."""
    L = len(dims)
    K0 = dims[0][1]
    f32 = arith == _F32
    if _tower_path_ok(M, in_width, dims, arith, on_gpu):
        # nothing has to be padded for the tower kernels: an input that arrives unpadded (13 dense features) is read with element loads; an
        # input that arrives padded to a multiple of 4 (the interaction's 367 -> 368 columns) meets a zero-padded copy of the first weight.
        # The per-layer forward GEMMs (no tower_fwd) pad an unaligned input as the per-layer path does
        pad_x = in_width == K0 and in_width % 4 != 0 and not TOWER_FWD
        Kp = in_width if in_width != K0 else _round4(K0) if pad_x else 0
        layers = (LayerPlan(dims[0][0], Kp or K0, acts[0], need_dx=need_dx), *[LayerPlan(dims[i][0], dims[i][1], acts[i]) for i in range(1, L)])
        return TowerPlan(layers, acts, arith, True, TOWER_FWD, None, in_width, pad_x, Kp, False, False, need_dx, False, consumer_act)
    # first layer: an input width that is no multiple of 4 floats runs on a zero-padded weight and a zero-padded input (x may already be one)
    Kp = _round4(K0) if K0 % 4 != 0 else 0
    if in_width != K0 and in_width != (Kp or K0):
        raise RuntimeError(_WIDTH_ERR % (in_width, K0))
    pad_x = Kp != 0 and in_width != Kp
    # sign bits: a forward that will be differentiated (Function.forward itself runs grad-free), and not a SMALL batch — there the GEMMs run
    # on 64 x 64 tiles that neither write nor read the bits (the bits would come from a stand-alone kernel: one more launch per layer of a
    # launch-bound step) and the data gradient reads the fp32 activation, which small batches keep in cache anyway
    need_bits = bool(RELU_BITS and need_grad and (M > SMALL_BATCH_BITS or (BF16_STORAGE and arith == _BF16) or
                                                  (BF16X6_PLANES and arith == _BF16X6)))
    # arith "bf16" with bf16 STORAGE (default; DLRM_BF16_STORAGE=0 restores the in-loop rounding of rounds 1-2): every GEMM layer reads a
    # bf16 copy of its input and of its weight (dlrm_gemm_bf16: no conversion in the k-loop).  LEAN (default, DLRM_BF16_LEAN=0 turns it
    # off): a hidden activation is written ONLY as bf16 + ReLU sign bits when every consumer reads those — the next layer's forward
    # GEMM, its weight gradient (dlrm_linear_bwd_weight_bf16 reads bf16 operands k-strided) and the data-gradient mask (sign bits); the
    # fp32 copy (4 of the 6 bytes written per element) exists only where something reads it: the tower's output, the input of a
    # matrix-vector layer, layers whose shapes the bf16 weight gradient does not take.  Same operand rounding and accumulation
    # order as the in-loop path for every product.
    # arith "bf16x6" with PLANES (default): the same plan with every bf16 copy replaced by the three planes of the fp32 tensor (always lean)
    st = _Bf16Store if (BF16_STORAGE and arith == _BF16) else None
    lean = st is not None and BF16_LEAN
    if BF16X6_PLANES and arith == _BF16X6 and M >= 256 and RELU_BITS and ops.BF16_PHASED:
        st, lean = _PlaneStore, True
    Ns = [N for N, _ in dims]
    Ks = [(Kp or K) if i == 0 else K for i, (_, K) in enumerate(dims)]
    mask = [ACT_NONE] + list(acts[:L - 1])                          # the derivative layer i's data gradient applies
    mbits = [i > 0 and mask[i] == ACT_RELU and need_bits for i in range(L)]
    dx = [i > 0 or need_dx for i in range(L)]
    if st is None:
        layers = tuple(LayerPlan(Ns[i], Ks[i], acts[i], bits=mbits[i + 1] if i + 1 < L else False, need_dx=dx[i], mask_act=mask[i],
                                 mask_bits=mbits[i]) for i in range(L))
        head = bool(HEAD_FUSED and Ns[-1] == 1 and L >= 2 and f32 and not consumer_act)
        return TowerPlan(layers, acts, arith, False, False, None, in_width, pad_x, Kp, need_bits, False, need_dx, head, consumer_act)
    kb = [st.kround(K) for K in Ks]
    fwd16 = [Ns[i] % 4 == 0 and Ns[i] != 1 and st.fwd_ok(M, Ns[i], kb[i]) for i in range(L)]
    if has_slot and not slot_aligned:
        fwd16[L - 1] = False
    # weight gradient of layer i from reduced-width operands as stored (the input of its forward GEMM, dZ16_i).  The input width asked
    # about is the PADDED one, where the tensor-level check at backward time (st.wgrad_ok) rounds the gradient's stored width up to 8:
    # for first-layer widths 57-60 the two differ (60 < 64 here, 64 there) and this, the stricter answer, is the one that decides
    wg16 = [bool(lean and need_grad and fwd16[i] and ops.linear_bwd_weight_bf16_shapes_ok(M, Ns[i], Ks[i])) for i in range(L)]
    # data gradient of layer i (dX = dZ . W) on reduced-width operands: reduction over N_i
    # (its epilogue applies the derivative of the activation BELOW it: none, or ReLU through that layer's sign bits)
    dg16 = [fwd16[i] and Ns[i] % 32 == 0 and Ks[i] % 4 == 0 and st.fwd_ok(M, Ks[i], Ns[i]) and (mask[i] == ACT_NONE or mbits[i]) for i in range(L)]
    out16 = [i + 1 < L and fwd16[i] and fwd16[i + 1] and kb[i + 1] == Ns[i] for i in range(L)]
    reads16 = [wg16[i] or (dg16[i] and dx[i]) for i in range(L)]    # backward of layer i reads its incoming gradient in reduced width
    # every weight copy of the tower in ONE launch (bf16 storage; the planes form keeps its per-layer splits): W16 [N, kb] for the forward
    # GEMM of a reduced-width layer, W^T16 [K, N] for its data gradient where backward will take that path (weights do not change in between)
    multi, w16m, wT16m = False, [False] * L, [False] * L
    if st is _Bf16Store and MULTI_CAST:
        wT = [need_grad and dg16[i] and dx[i] for i in range(L)]
        if sum(fwd16[i] or wT[i] for i in range(L)) > 1:
            multi, w16m, wT16m = True, fwd16, wT
    layers = []
    for i in range(L):
        # the fp32 output: not lean, the tower's output, or the next layer's forward GEMM does not take the reduced-width one as it is ...
        out32 = (not lean) or not out16[i]
        if not out32 and need_grad:
            # ... or a backward consumer reads it: the next layer's weight gradient when it is not the reduced-width one; its DATA gradient
            # when it is not (widths the bf16 / plane GEMM refuses, e.g. 200 or 72: the fp32-storage fallback, ops.linear_bwd_data, masks
            # with this activation, the sign bits alone would not do); the ReLU derivative when there are no sign bits; any other
            # activation's derivative
            out32 = (not wg16[i + 1]) or (not dg16[i + 1]) or (acts[i] == ACT_RELU and not need_bits) or acts[i] not in (ACT_RELU, ACT_NONE)
        # what the layer below reads of this layer's data gradient: its reduced-width weight / data gradient take the reduced-width copy;
        # fp32 is written only when something reads it (the tower's input gradient, an fp32-storage weight / data gradient below)
        want16 = i > 0 and reads16[i - 1] and Ks[i] % 32 == 0
        want32 = i == 0 or not want16 or not (wg16[i - 1] and (dg16[i - 1] or not dx[i - 1]))
        layers.append(LayerPlan(Ns[i], Ks[i], acts[i], out32, fwd16[i], kb[i], out16[i], mbits[i + 1] if i + 1 < L else False, w16m[i], wT16m[i],
                                wg16[i], dx[i], dg16[i], want32 or not dg16[i], want16 and dg16[i], mask[i], mbits[i]))    # (in field order)
    return TowerPlan(tuple(layers), acts, arith, False, False, st, in_width, pad_x, Kp, need_bits, multi, need_dx, False, consumer_act)


class MLPFunction(Function):
    """nn.Sequential(Linear, act, Linear, act, ...) as one chain of fused GEMM(+bias+act) kernels.

    forward(x, acts, out_slot, arith, W0, b0, W1, b1, ...) -> activated output of the last layer (`arith`: the MLP
    arithmetic of every GEMM of the tower, forward and backward — a per-call argument of the C ABI).
    Reference: DLRM_Net.create_mlp / apply_mlp (dlrm_s_pytorch.py:208-246, 399-405).

    Input widths that are not a multiple of 4 floats (13 dense features, 479 interaction outputs) would
    force 4-byte loads in the first GEMM: the first layer then runs on a zero-padded copy of its weight
    [N, round4(K)] and on a zero-padded input.  `x` may already BE that padded input (width round4(K) with
    zero padding columns, which is what InteractFunction(padded=True) emits); otherwise a padded copy of
    `x` is made (cheap: it only happens for the narrow dense-feature input)."""

    @staticmethod
    def forward(ctx, x, acts, out_slot, arith, *params):
        x = _rowmajor(x)
        # MLP_CONSUMER_APPLIES_LAST_ACT OR-ed into `arith`: the gradient this tower receives is already multiplied by the derivative of its
        # LAST activation (a ReLU) — the interaction backward does that to its feature-0 gradient on request (ops.INTERACT_RELU_X), so
        # backward starts from dY as it comes instead of with an act_bwd pass over [M, N_last]
        consumer_act = bool(int(arith) & MLP_CONSUMER_APPLIES_LAST_ACT)
        arith = int(arith) & ~MLP_CONSUMER_APPLIES_LAST_ACT
        if consumer_act and acts[-1] != ACT_RELU:
            raise RuntimeError("dlrm_amd: MLP_CONSUMER_APPLIES_LAST_ACT needs a tower that ends in a ReLU")
        L = len(acts)
        M = x.size(0)
        out_last = out_slot.get() if out_slot is not None else None
        plan = _plan_tower(M, x.size(1), [params[2 * i].shape for i in range(L)], acts, arith,
                           any(ctx.needs_input_grad), ctx.needs_input_grad[0], x.is_cuda, out_last is not None,
                           out_last is None or (_ld(out_last) % 4 == 0 and out_last.data_ptr() % 16 == 0), consumer_act)
        ctx.plan = plan
        # first-layer padding, the one place: Ws[i] is the weight layer i's GEMMs run on, forward and backward
        Ws = [params[2 * i] for i in range(L)]
        W0p = None
        if plan.Kp:
            if plan.pad_x:
                x = ops.pad_cols(x, plan.Kp)
            W0p = Ws[0] = ops.pad_cols(Ws[0], plan.Kp)
        if plan.whole_tower:
            outs = MLPFunction._tower_forward(plan, x, out_last, Ws, params)
        else:
            outs = MLPFunction._layers_forward(ctx, plan, x, out_last, Ws, params)
        ctx.save_for_backward(x, *params, *[o for o in outs if o is not None], *([W0p] if W0p is not None else []))
        return outs[-1]

    @staticmethod
    def _saved(ctx):
        """x as the first layer read it, the parameters, every layer's fp32 output (None: the layer kept reduced width + sign bits only) and
        the weights the GEMMs run on"""
        layers = ctx.plan.layers
        L = len(layers)
        saved = ctx.saved_tensors
        rest = iter(saved[1 + 2 * L:])
        outs = [next(rest) if lp.out32 else None for lp in layers]
        Ws = [saved[1 + 2 * i] for i in range(L)]
        if ctx.plan.Kp:
            Ws[0] = next(rest)
        return saved[0], saved[1:1 + 2 * L], outs, Ws

    @staticmethod
    def _layers_forward(ctx, plan, x, out_last, Ws, params):
        st, acts, layers = plan.store, plan.acts, plan.layers
        L = len(layers)
        M = x.size(0)
        pre16, preT16 = [None] * L, [None] * L
        if plan.multi_cast:
            where = [i for i, lp in enumerate(layers) if lp.w16_multi or lp.wT16_multi]
            items = [(Ws[i], layers[i].kb if layers[i].w16_multi else None, layers[i].N if layers[i].wT16_multi else None) for i in where]
            for i, (d_, dT_) in zip(where, st.cast_multi(items, category="linear_fwd")):
                pre16[i], preT16[i] = d_, dT_
        cur, cur16 = x, None                                            # the current activation: fp32, and its reduced-width copy [M, kb of the next layer]
        outs, in16, bits = [], [], []                                   # in16[i]: the reduced-width input of layer i's GEMM, kept for its weight gradient
        for i, lp in enumerate(layers):
            b = params[2 * i + 1]
            y = (out_last if (i == L - 1 and out_last is not None) else alloc2d(M, lp.N, x)) if lp.out32 else None
            # hidden ReLU layers also store their sign bits (1 bit per element): the data-gradient GEMM of the NEXT layer reads
            # those instead of this fp32 activation for its fused ReLU derivative
            rb = ops.relu_bits_alloc(M, lp.N, x.device) if lp.bits else None
            y16 = None
            if lp.fwd16:
                a16 = cur16 if cur16 is not None else st.cast(cur, lp.kb, category="linear_fwd")
                in16.append(a16 if lp.wgrad16 else None)
                w16 = pre16[i] if pre16[i] is not None else st.cast(Ws[i], lp.kb, category="linear_fwd")
                y16 = st.empty(M, lp.N, x.device) if lp.out16 else None
                st.gemm(a16, w16, b, acts[i], y, y16, relu_bits_out=rb, category="linear_fwd")
            else:
                in16.append(None)
                ops.linear_fwd(cur, Ws[i], b, acts[i], y, plan.arith, relu_bits=rb)
            cur, cur16 = y, y16
            outs.append(y)
            bits.append(rb)
        ctx.in16, ctx.bits, ctx.preT16 = in16, bits, preT16
        return outs

    @staticmethod
    def _tower_forward(plan, x, out_last, Ws, params):
        """small batches, native fp32: this tower's BACKWARD pass will run on the whole-tower kernels of csrc/tower.hip (one launch for the
        data-gradient chain, one + one for all weight / bias gradients), so every layer's fp32 output is kept.  The forward pass is the
        per-layer GEMMs by default (which spread a layer over the whole chip), or (TOWER_FWD) one tower launch — activations of 16 batch
        rows stay in LDS from layer to layer."""
        L = len(plan.layers)
        M = x.size(0)
        outs = [(out_last if (i == L - 1 and out_last is not None) else alloc2d(M, lp.N, x)) for i, lp in enumerate(plan.layers)]
        if plan.tower_fwd:
            ops.tower_fwd(x, Ws, [params[2 * i + 1] for i in range(L)], plan.acts, outs)
        else:
            cur = x
            for i in range(L):
                ops.linear_fwd(cur, Ws[i], params[2 * i + 1], plan.acts[i], outs[i], ops.arith_code("f32"), relu_bits=None)
                cur = outs[i]
        return outs

    @staticmethod
    def _tower_backward(ctx, dY):
        plan = ctx.plan
        L = len(plan.layers)
        x, params, outs, Ws = MLPFunction._saved(ctx)
        M = x.size(0)
        dY = _rowmajor(dY)
        dZs = [alloc2d(M, lp.N, x) for lp in plan.layers]
        dX = alloc2d(M, x.size(1), x) if plan.need_dx else None
        ops.tower_bwd(dY, Ws, plan.acts, outs, dZs, dX, last_act_applied=plan.consumer_act)
        dWs = [_grad_out(params[2 * i]) for i in range(L)]              # (the first layer's at the parameter's true width)
        dbs = [_grad_out(params[2 * i + 1]) for i in range(L)]
        ops.tower_wgrad(dZs, [x] + outs[:-1], dWs, dbs)
        grads = []
        for i in range(L):
            grads += [dWs[i], dbs[i]]
        if dX is not None and dX.size(1) != plan.in_width:
            dX = dX[:, :plan.in_width]
        return (dX, None, None, None, *grads)

    @staticmethod
    def backward(ctx, dY):
        plan = ctx.plan
        if plan.whole_tower:
            return MLPFunction._tower_backward(ctx, dY)
        st, acts, arith, layers = plan.store, plan.acts, plan.arith, plan.layers
        L = len(layers)
        x, params, outs, Ws = MLPFunction._saved(ctx)
        M = x.size(0)
        dY = _rowmajor(dY)
        grads: List[Optional[torch.Tensor]] = [None] * (2 * L)
        overlap = _wgrad_overlaps(M)

        # last layer: activation backward (its dY comes from outside, e.g. the loss or the interaction)
        first = L - 1                                      # the layer the loop below starts with
        dZ = None
        if plan.head_fused and not overlap:
            # the 256 -> 1 head of the top tower: act_bwd + weight gradient + data gradient of an N == 1 layer are ONE pass over its input
            # (dlrm_linear_head_bwd: X read once instead of twice, one launch + the finish instead of four: 48 -> ~29 us at B = 65536; the
            # bits of the three calls).  Outside its fast path nothing is launched and the three calls below run.
            dW_h, db_h = _grad_out(params[2 * (L - 1)]), _grad_out(params[2 * (L - 1) + 1])
            dprev = alloc2d(M, layers[L - 1].K, x)
            if ops.linear_head_bwd(dY, outs[L - 1], acts[L - 1], outs[L - 2], Ws[L - 1], acts[L - 2], dprev, dW_h, db_h):
                grads[2 * (L - 1)], grads[2 * (L - 1) + 1] = dW_h, db_h
                dZ, first = dprev, L - 2
        if dZ is not None:
            pass
        elif plan.consumer_act and _ld(dY) % 4 == 0 and dY.data_ptr() % 16 == 0:
            dZ = dY                                        # already dL/dz of the last layer (see forward)
        else:
            dZ = alloc2d(M, layers[L - 1].N, x)
            if plan.consumer_act:
                dZ.copy_(dY)                               # (an unaligned gradient view: the GEMMs want 16-byte rows)
            else:
                ops.act_bwd(dY, outs[L - 1], acts[L - 1], dZ, None)
        dX = None
        # The weight-gradient GEMM of layer i and the data-gradient GEMM that feeds layer i-1 both consume dZ_i and
        # are independent: wgrad goes to a side HIP stream so the two kernels share the chip (their epilogue
        # store bursts and tail rounds interleave with the other's MFMA phases instead of idling the matrix cores).
        main = torch.cuda.current_stream()
        side = _side_stream(x.device) if overlap else None
        keep = []                                          # tensors the side stream reads stay alive until the join
        dZ16 = None                                        # reduced-width copy of dZ when the previous data-gradient GEMM produced one
        for i in range(first, -1, -1):
            lp, W = layers[i], Ws[i]
            X_i = x if i == 0 else outs[i - 1]
            X16_i = ctx.in16[i]
            # first layer on a zero-padded input: the gradient is written at the parameter's true width (the padding
            # columns of X are dropped inside the kernel) — contiguous, no slicing / re-packing afterwards
            dW = _grad_out(params[2 * i])
            db = _grad_out(params[2 * i + 1])
            # the one check of the plan that needs the real gradient slot (it may be a view into a flat all-reduce buffer)
            if lp.wgrad16 and not st.wgrad_ok(M, lp.N, dW.size(1), dZ16 if dZ16 is not None else X16_i, X16_i):
                # forward already dropped the fp32 operands on the strength of this plan: a run-time disagreement (DLRM_BF16_PHASED changed
                # between forward and backward, an unaligned gradient slot) must not fall into the fp32 branch with operands that no longer exist
                raise RuntimeError("dlrm_amd: the bf16 weight gradient planned at forward time for layer %d (M=%d, N=%d, K=%d) is refused at "
                                   "backward time (environment switched between forward and backward, or unaligned gradient storage)"
                                   % (i, M, lp.N, dW.size(1)))
            if lp.wgrad16 and dZ16 is None:
                dZ16 = st.cast(dZ, lp.N, category="linear_bwd_weight")               # (the tower's last layer: its dZ comes from act_bwd in fp32)

            def wgrad():
                if lp.wgrad16:
                    st.wgrad(dZ16, X16_i, dW, db)                                 # bf16 operands (or planes) as stored, k-strided reads
                else:
                    ops.linear_bwd_weight(dZ, X_i, dW, db, arith=arith)           # dW and db (row sums of dZ^T) in one GEMM
            if side is not None:
                side.wait_event(main.record_event())
                with torch.cuda.stream(side):
                    wgrad()
                keep += [dZ, dZ16]
            else:
                wgrad()
            grads[2 * i], grads[2 * i + 1] = dW, db
            if not lp.need_dx:
                continue
            rbits = ctx.bits[i - 1] if i > 0 else None
            dprev = alloc2d(M, lp.K, x) if lp.dx32 else None
            if lp.dgrad16:
                # reduced-width storage: dX = dZ . W as a <k-contiguous, k-contiguous> GEMM over a transposed reduced-width copy of W
                a16 = dZ16 if dZ16 is not None else st.cast(dZ, lp.N, category="linear_bwd_data")
                wT16 = ctx.preT16[i] if ctx.preT16[i] is not None else st.cast_t(W, lp.N, category="linear_bwd_data")
                d16 = st.empty(M, lp.K, x.device) if lp.dx16 else None
                st.gemm(a16, wT16, None, ACT_NONE, dprev, d16, relu_bits_in=rbits, category="linear_bwd_data")
                dZ16 = d16
            else:
                # dgrad GEMM with the previous layer's activation derivative fused into the epilogue
                if dZ is None:
                    raise RuntimeError("dlrm_amd: internal: fp32 gradient missing for an fp32-storage data gradient")
                ops.linear_bwd_data(dZ, W, X_i if i > 0 else None, lp.mask_act, dprev, arith, relu_bits=rbits)
                dZ16 = None
            if i > 0:
                dZ = dprev
            else:
                dX = dprev
                if dX.size(1) != plan.in_width:
                    dX = dX[:, :plan.in_width]
        if side is not None:
            main.wait_stream(side)
            del keep
        return (dX, None, None, None, *grads)


_NO_SINK = "dlrm_amd: embedding backward needs a gradient sink (fused update)"
_NO_QR_SUMS = "dlrm_amd: this QR lookup ran without gradients enabled; its pooled sums were not kept"


def _qr_tables(vweights, collisions):
    """the VIRTUAL table list (weight_q then weight_r of a QR table, the weight of a plain one) -> (weights, weights_r), None for a plain table's r"""
    it = iter(vweights)
    weights, weights_r = [], []
    for c in collisions:
        weights.append(next(it))
        weights_r.append(next(it) if c else None)
    return weights, weights_r


class EmbeddingBagsFunction(Function):
    """All T EmbeddingBag(sum) lookups in one kernel launch; the backward pass does NOT materialise a
    gradient: it hands (bags, d_out) to `sink`, which applies the fused sparse update when the
    optimizer steps.  Reference: DLRM_Net.apply_emb (dlrm_s_pytorch.py:407-462).
    Tables all fp32, or all torch.bfloat16 (DLRM_Net.embedding_bfloat16: dlrm_emb_fwd_bf16 pools them into the fp32 feature buffer — the bits
    of the fp32 lookup on the upcast tables; the model routes what backward hands to `sink` to the bf16 update kernels)."""

    @staticmethod
    def forward(ctx, sink, bags, out_slot, *tensors):
        # tensors = the T tables, optionally followed by T pooling-weight vectors [rows_t] (--weighted-pooling: `v_W_l`,
        # dlrm_s_pytorch.py:289-293,370-375): psw = v_W[idx] is gathered here and, when the vectors are Parameters
        # ("learned"), their dense gradient comes back from backward
        T = bags.T
        weights, vws = tensors[:T], tensors[T:]
        D = weights[0].size(1)
        bf16 = weights[0].dtype == torch.bfloat16          # (a mixture is refused by the lookup's table description)
        if vws:
            if bf16 and any(v.requires_grad for v in vws):
                # (the gradient kernel of learned vectors reads fp32 rows; the model refuses them before it gets here)
                raise RuntimeError("dlrm_amd: learned pooling weights are not built for bfloat16 embedding tables")
            ops.pool_weights_gather(vws, bags)
        out = out_slot.get() if out_slot is not None else alloc2d(bags.B, T * D, weights[0])        # (fp32, on the tables' device)
        (ops.emb_fwd_bf16 if bf16 else ops.emb_fwd)(weights, bags, out)
        ctx.sink = sink
        ctx.bags = bags
        ctx.weights = weights  # parameters (leaves) — kept by reference, not via save_for_backward
        ctx.vws = vws
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.sink is None:
            raise RuntimeError(_NO_SINK)
        dout = _rowmajor(dout)
        dvw = (None,) * len(ctx.vws)
        if ctx.vws and any(ctx.needs_input_grad[3 + len(ctx.weights):]):
            dvw = tuple(ops.emb_psw_grad(ctx.weights, ctx.bags, dout, ctx.vws))    # before the update touches the tables
        ctx.sink(ctx.weights, ctx.bags, dout)
        return (None, None, None) + (None,) * len(ctx.weights) + dvw


class QREmbeddingBagsFunction(Function):
    """EmbeddingBagsFunction for a table list with quotient-remainder tables (tricks/qr_embedding_bag.py; dlrm_s_pytorch.py:258-266): one
    dlrm_emb_fwd_qr launch pools every table, QR or plain.  spec = (rows, collisions, operation, keep_sums); `vweights` is the VIRTUAL table
    list — weight_q then weight_r for a QR table, the weight of a plain one.  Backward runs one streaming pass (dlrm_emb_qr_bwd_split) from
    d_out and the two pooled sums the forward kept to the gradient buffer of the virtual list, derives the q / r ids
    (dlrm_emb_qr_split_indices) and hands (virtual weights, virtual bags, buffer) to `sink`: the sparse updates are the existing ones."""

    @staticmethod
    def forward(ctx, sink, bags, out_slot, spec, *vweights):
        rows, collisions, op, keep_sums = spec
        weights, weights_r = _qr_tables(vweights, collisions)
        D = weights[0].size(1)
        out = out_slot.get() if out_slot is not None else alloc2d(bags.B, bags.T * D, weights[0])
        saved = None
        if keep_sums and op == "mult":
            saved = torch.empty((bags.B, 2 * D * sum(1 for c in collisions if c)), dtype=torch.float32, device=out.device)
        ops.emb_fwd_qr(weights, weights_r, rows, collisions, op, bags, out, saved)
        ctx.sink, ctx.bags, ctx.spec, ctx.D = sink, bags, spec, D
        ctx.vweights = vweights      # parameters (leaves) — kept by reference, not via save_for_backward
        ctx.saved = saved
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.sink is None:
            raise RuntimeError(_NO_SINK)
        rows, collisions, op, _ = ctx.spec
        if op == "mult" and ctx.saved is None:
            raise RuntimeError(_NO_QR_SUMS)
        gout = ops.emb_qr_bwd_split(collisions, op, ctx.D, _rowmajor(dout), ctx.saved)     # (the sums stay with the node: a retained graph may run again)
        ctx.sink(ctx.vweights, ops.qr_virtual_bags(rows, collisions, ctx.bags), gout)
        return (None, None, None, None) + (None,) * len(ctx.vweights)


class MDEmbeddingBagsFunction(Function):
    """EmbeddingBagsFunction for a table list with mixed-dimension tables (tricks/md_embedding_bag.py PrEmbeddingBag; dlrm_s_pytorch.py:267-275):
    one dlrm_emb_fwd_md launch pools every table at its own width and projects it to the common width D.  spec = (D, has_proj, keep_sums);
    `tensors` = the T tables, then the [D, d_t] projection weight of every table with has_proj[t], in table order.  Backward is one
    dlrm_emb_md_bwd call: the dense projection gradients come back as the gradients of the projection inputs, and the gradient of the pooled
    sums — laid out by ops.MDLayout, tables of equal width contiguous — is handed to `sink` once per width, with that group's tables and bags:
    the sparse updates are the existing ones."""

    @staticmethod
    def forward(ctx, sink, bags, out_slot, spec, *tensors):
        D, has_proj, keep_sums = spec
        T = bags.T
        weights = tensors[:T]
        it = iter(tensors[T:])
        projs = [next(it) if h else None for h in has_proj]
        layout = ops.MDLayout([w.size(1) for w in weights])
        out = out_slot.get() if out_slot is not None else alloc2d(bags.B, T * D, weights[0])
        saved = torch.empty((bags.B, layout.width), dtype=torch.float32, device=out.device) if keep_sums else None
        ops.emb_fwd_md(weights, projs, D, bags, out, saved, layout.cols if keep_sums else None)
        ctx.sink, ctx.bags, ctx.D, ctx.layout = sink, bags, D, layout
        ctx.weights, ctx.projs = weights, projs      # parameters (leaves) — kept by reference, not via save_for_backward
        ctx.saved = saved
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.sink is None:
            raise RuntimeError(_NO_SINK)
        T, layout = len(ctx.weights), ctx.layout
        need = iter(ctx.needs_input_grad[4 + T:])
        want = [p_ is not None and next(need) for p_ in ctx.projs]
        dout = _rowmajor(dout)
        gout = torch.empty((dout.size(0), layout.width), dtype=torch.float32, device=dout.device)
        _, dprojs = ops.emb_md_bwd(ctx.projs, layout.dims, ctx.D, dout, ctx.saved, layout.cols, gout, want)   # (the sums stay with the node)
        for d, ks, c0 in layout.groups:
            ctx.sink(tuple(ctx.weights[k] for k in ks), ops.bag_subset(ctx.bags, ks), gout[:, c0:c0 + len(ks) * d])
        return (None, None, None, None) + (None,) * T + tuple(g for g, p_ in zip(dprojs, ctx.projs) if p_ is not None)


class InteractFunction(Function):
    """R = [x | strictly-lower-triangular pairwise dots of the F feature vectors].

    forward(D, self_interaction, padded, block0, block1, ...): each block is [B, k*D] and contributes k
    features (block0 = bottom-MLP output).  Reference: interact_features (dlrm_s_pytorch.py:483-504)."""

    @staticmethod
    def forward(ctx, D, self_interaction, padded, *blocks):
        order = None
        if blocks and isinstance(blocks[0], (list, tuple)):          # optional leading feature permutation (see ops.interact_fwd)
            order, blocks = list(blocks[0]), blocks[1:]
        blocks = tuple(_rowmajor(b) for b in blocks)
        B = blocks[0].size(0)
        F = sum(b.size(1) // D for b in blocks)
        # `self_interaction | ops.INTERACT_RELU_X` (backward only): block 0's first feature is a ReLU output whose derivative the backward
        # kernel applies (the producing MLPFunction was told so: MLP_CONSUMER_APPLIES_LAST_ACT) — never together with a permutation
        relu_x = int(self_interaction) & ops.INTERACT_RELU_X
        if relu_x and order is not None:
            raise RuntimeError("dlrm_amd: INTERACT_RELU_X names feature 0 of the block list; it cannot be combined with a feature permutation")
        mode = int(self_interaction) & 3
        Wd = ops.interact_out_width(F, D, mode)
        ldr = _round4(Wd)
        Rfull = torch.empty((B, ldr), dtype=torch.float32, device=blocks[0].device)
        ops.interact_fwd(blocks, D, mode, Rfull, order=order)
        ctx.order = order
        ctx.D, ctx.self_interaction, ctx.width = D, mode | relu_x, Wd
        ctx.save_for_backward(*blocks)
        # padded=True hands out the whole [B, round4(width)] buffer (zero padding columns) for MLPFunction
        return Rfull if (ldr == Wd or padded) else Rfull[:, :Wd]

    @staticmethod
    def backward(ctx, dR):
        blocks = ctx.saved_tensors
        dR = _rowmajor(dR)
        B = blocks[0].size(0)
        total = sum(b.size(1) for b in blocks)
        # one flat buffer, one contiguous [B, k*D] chunk per input block, in input order: the chunks of the
        # all-to-all outputs are therefore already the packed send buffer of the reverse exchange
        flat = torch.empty(B * total, dtype=torch.float32, device=dR.device)
        dblocks, o = [], 0
        for b in blocks:
            n = B * b.size(1)
            dblocks.append(flat[o:o + n].view(B, b.size(1)))
            o += n
        ops.interact_bwd(blocks, ctx.D, ctx.self_interaction, dR, dblocks, order=ctx.order)
        return (None, None, None, *dblocks) if ctx.order is None else (None, None, None, None, *dblocks)


class ProjectInteractFunction(Function):
    """R = [x | Z flattened row-major], Z[b] = P1[b].view(I1, D) @ P2[b].view(D, I2) — the projected interaction of torchrec's
    DLRM_Projection (ops.proj_interact_fwd / proj_interact_bwd; fp32).

    forward(D, padded, x, P1, P2): x [B, D] is read in place (a column slice of the feature buffer), P1 [B, I1*D], P2 [B, D*I2]."""

    @staticmethod
    def forward(ctx, D, padded, x, P1, P2):
        x, P1, P2 = _rowmajor(x), _rowmajor(P1), _rowmajor(P2)
        B = x.size(0)
        I1, I2 = ops._proj_dims(P1, P2, D)
        Wd = D + I1 * I2
        ldr = _round4(Wd)
        Rfull = torch.empty((B, ldr), dtype=torch.float32, device=x.device)
        ops.proj_interact_fwd(x, P1, P2, D, Rfull)
        ctx.D = D
        ctx.save_for_backward(P1, P2)
        # padded=True hands out the whole [B, round4(width)] buffer (zero padding columns) for MLPFunction
        return Rfull if (ldr == Wd or padded) else Rfull[:, :Wd]

    @staticmethod
    def backward(ctx, dR):
        P1, P2 = ctx.saved_tensors
        dR = _rowmajor(dR)
        B, D = P1.size(0), ctx.D
        # one flat buffer, one contiguous chunk per input, in input order (x, P1, P2)
        widths = (D, P1.size(1), P2.size(1))
        flat = torch.empty(B * sum(widths), dtype=torch.float32, device=dR.device)
        grads, o = [], 0
        for w in widths:
            grads.append(flat[o:o + B * w].view(B, w))
            o += B * w
        ops.proj_interact_bwd(P1, P2, D, dR, *grads)
        return (None, None, *grads)


class GatherKind(NamedTuple):
    """What the fused lookup + interaction path needs to know of a route's kind (dlrm_net.fused_route): a key of ops.ROW_KINDS, or "fp32".
    The wrappers are NAMES of `ops` attributes, looked up when they are called."""
    fwd: str
    bwd: Optional[str]          # None: forward only (packed tables are constants; their table description holds D)
    lookup: str                 # the lookup of the two-kernel form behind (flag, 1)
    virtual: bool = False       # QR: the sink takes the VIRTUAL table list, its [B, Tv*D] buffer (emb_qr_bwd_split behind (flag, 1)) and qr_virtual_bags
    presort: bool = False       # `bags.presort` is read: the update inside the backward


# (fp32 and bf16 at D = 128 name the same wrappers: ops.interact_*_gather dispatch on the tables' dtype themselves)
GATHER_KINDS = {
    "fp32": GatherKind("interact_fwd_gather", "interact_bwd_gather", "emb_fwd", presort=True),
    "bf16": GatherKind("interact_fwd_gather", "interact_bwd_gather", "emb_fwd_bf16"),
    "narrow": GatherKind("interact_fwd_gather_narrow", "interact_bwd_gather_narrow", "emb_fwd"),
    "narrow_bf16": GatherKind("interact_fwd_gather_narrow_bf16", "interact_bwd_gather_narrow_bf16", "emb_fwd_bf16"),
    "qr": GatherKind("interact_fwd_gather_qr", "interact_bwd_gather_qr", "emb_fwd_qr", virtual=True),
    "narrow_qr": GatherKind("interact_fwd_gather_narrow_qr", "interact_bwd_gather_narrow_qr", "emb_fwd_qr", virtual=True),
    "quant": GatherKind("interact_fwd_gather_quant", None, "emb_fwd_quant"),
    "narrow_quant": GatherKind("interact_fwd_gather_narrow_quant", None, "emb_fwd_quant"),
}


def gather_interact_fwd(ctx, sink, kind, spec, D, self_interaction, bags, x, tables):
    """The forward of the fused lookup + interaction path, for GatherInteractFunction and, with ctx = None, for the packed routes, which need no
    autograd node: R [B, round4(width)] = interaction of [x | one row per bag of the tables of `kind`].
    spec: None for plain tables; (rows, collisions, operation, keep_sums) with `tables` the VIRTUAL list for QR ones, as QREmbeddingBagsFunction
    takes them; (rows, D, bits) for packed ones.
    `bags.iota_flag` (a device int32, ops.offsets_iota_state in dlrm_amd/iota.py): whether the batch really has ONE lookup per bag is known on the
    device only — nnz == B does not prove it.  Absent: the fused call runs alone.  Present: both implementations are enqueued with that launch
    predicate (ABI 16) — the fused call runs if the flag is zero; the lookup + the plain interaction (the reference's apply_emb +
    interact_features as two kernels, through a pooled buffer ly that then has to live until backward; QR: and the two pooled sums) run if it is
    not.  The launches that do not run return at once; the host never waits."""
    k = GATHER_KINDS[kind]
    x = _rowmajor(x)
    B, sums = x.size(0), 0
    if k.virtual:
        rows, collisions, op, keep_sums = spec
        t = (*_qr_tables(tables, collisions), rows, collisions, op)
        T = len(collisions)
        if keep_sums and op == "mult":
            sums = 2 * D * sum(1 for c in collisions if c)
    else:
        t, T = (tables,) if spec is None else (tables, *spec), len(tables)
    mode = int(self_interaction) & 3                      # (| ops.INTERACT_RELU_X: see InteractFunction.forward)
    R = torch.empty((B, _round4(ops.interact_out_width(1 + T, D, mode))), dtype=torch.float32, device=x.device)
    flag = getattr(bags, "iota_flag", None)
    fwd = getattr(ops, k.fwd)
    out = (bags, mode, R) if k.bwd is None else (bags, D, mode, R)
    ly = saved = None
    if flag is None:
        fwd(x, *t, *out, pred=None)
    else:
        fwd(x, *t, *out, pred=(flag, 0))
        ly = alloc2d(B, T * D, x)
        if k.virtual:
            if sums:
                saved = torch.empty((B, sums), dtype=torch.float32, device=x.device)
            getattr(ops, k.lookup)(*t, bags, ly, saved, pred=(flag, 1))
        else:
            getattr(ops, k.lookup)(*t, bags, ly, pred=(flag, 1))
        ops.interact_fwd((x, ly), D, mode, R, pred=(flag, 1))
    if ctx is not None:
        ctx.sink, ctx.bags, ctx.flag, ctx.kind = sink, bags, flag, kind
        ctx.D, ctx.T, ctx.self_interaction = D, T, int(self_interaction) & (3 | ops.INTERACT_RELU_X)
        ctx.tables, ctx.t, ctx.saved = tables, t, saved      # parameters (leaves) — kept by reference, not via save_for_backward
        ctx.save_for_backward(*((x,) if ly is None else (x, ly)))
    return R                                   # zero padding columns (what MLPFunction takes as is)


def _flat_dx_dE(B, D, T, device):
    """dx [B, D] | dE [B, T*D] out of one allocation"""
    flat = torch.empty(B * (1 + T) * D, dtype=torch.float32, device=device)
    return flat[:B * D].view(B, D), flat[B * D:].view(B, T * D)


class GatherInteractFunction(Function):
    """apply_emb + interact_features fused for one-lookup-per-bag batches (dlrm_s_pytorch.py:407-462 + 483-504), for every kind of
    GATHER_KINDS with a backward: R = [x | lower-triangular dots of (x, the row of table 1, ..., the row of table T)], the rows fetched (QR:
    and composed) by the interaction kernel itself — the bits of the kind's *EmbeddingBagsFunction + InteractFunction, without the [B, T*D]
    pooled-embedding buffer (QR: its gradient and the [B, 2*Tq*D] pooled sums).  apply(sink, kind, spec, D, mode, bags, x, *tables): see
    gather_interact_fwd.  Backward recomputes nothing: it gathers the same rows again, writes dx and the gradient of the gathered rows, and
    hands the latter to `sink` (the fused sparse update) exactly as the kind's *EmbeddingBagsFunction.backward does: one update call per step,
    with or without a flag."""

    @staticmethod
    def forward(ctx, sink, kind, spec, D, self_interaction, bags, x, *tables):
        return gather_interact_fwd(ctx, sink, kind, spec, D, self_interaction, bags, x, tables)

    @staticmethod
    def backward(ctx, dR):
        if ctx.sink is None:
            raise RuntimeError(_NO_SINK)
        k = GATHER_KINDS[ctx.kind]
        x = ctx.saved_tensors[0]
        dR = _rowmajor(dR)
        B, D, T, t, bags, flag = x.size(0), ctx.D, ctx.T, ctx.t, ctx.bags, ctx.flag
        if k.virtual:
            collisions, op = t[3], t[4]
            dx = torch.empty((B, D), dtype=torch.float32, device=dR.device)
            dE = torch.empty((B, len(ctx.tables) * D), dtype=torch.float32, device=dR.device)       # `gout`, the buffer of the virtual list
        else:
            dx, dE = _flat_dx_dE(B, D, T, dR.device)
        pred = None if flag is None else (flag, 0)
        # `bags.presort` (DLRM_Net._presort_for_backward; None unless the model was told to update in backward and knows its SGD optimizer): the
        # sort of the sparse update runs NOW and the fused kernel takes the SGD step of every row a single lookup of the batch names (its table
        # row is staged in LDS anyway) — ops.Presorted travels to the sink, which applies the rest from the same sorted workspace
        presort = getattr(bags, "presort", None) if k.presort else None
        pre = presort(ctx.tables, bags, pred) if presort is not None else None
        more = {} if pre is None else {"presorted": pre}
        getattr(ops, k.bwd)(x, *t, bags, D, ctx.self_interaction, dR, dx, dE, pred=pred, **more)
        if flag is not None:
            # ... and behind (flag, 1) the plain interaction backward over (x, the saved pooled buffer)
            pooled = dE
            if k.virtual:
                if op == "mult" and ctx.saved is None:
                    raise RuntimeError(_NO_QR_SUMS)
                pooled = torch.empty((B, T * D), dtype=torch.float32, device=dR.device)
            ops.interact_bwd((x, ctx.saved_tensors[1]), D, ctx.self_interaction, dR, (dx, pooled), pred=(flag, 1))
            if k.virtual:
                ops.emb_qr_bwd_split(collisions, op, D, pooled, ctx.saved, dE, pred=(flag, 1))
        ctx.sink(ctx.tables, ops.qr_virtual_bags(t[2], collisions, bags) if k.virtual else bags, dE, **more)
        return (None, None, None, None, None, None, dx) + (None,) * len(ctx.tables)


class LowRankCrossNetFunction(Function):
    """DCN-v2 interaction (torchrec.modules.crossnet.LowRankCrossNet, the MLPerf-v2 default: torchrec_dlrm/dlrm_main.py:608-619):
        x_{l+1} = x_0 * (W_l (V_l x_l) + b_l) + x_l,   l = 0 .. L-1,   on the flattened feature buffer x_0 [B, F*D].
    forward(arith, x0, V_0, W_0, b_0, V_1, ...): V_l [r, in], W_l [in, r], b_l [in].  Both products run on the MLP GEMM kernels
    (act none), the elementwise halves on dlrm_cross_fwd / _bwd; backward is written out by hand so that the three gradient
    streams into x_0 (through every layer's Hadamard factor, and through x_l of layer 0) are accumulated by our kernels instead
    of autograd's ATen adds."""

    @staticmethod
    def _bf16_ok(arith, M, n_in, r) -> bool:
        """bf16 STORAGE form (arith "bf16"): every product reads bf16 operands as stored — x_l and du as the bf16 copies the elementwise
        kernels write beside (or instead of) their fp32 results, v and dv as bf16-only GEMM outputs; weight gradients from the stored
        operands (dlrm_linear_bwd_weight_bf16); the gradient sum g + dv.V inside the GEMM epilogue (addend).  Needs the shapes of the
        bf16-shaped kernels."""
        return (BF16_STORAGE and BF16_LEAN and arith == ops.arith_code("bf16") and n_in % 64 == 0 and r % 64 == 0 and n_in >= 192 and r >= 192
                and ops.linear_bwd_weight_bf16_shapes_ok(M, r, n_in) and ops.linear_bwd_weight_bf16_shapes_ok(M, n_in, r))   # dV [r, in], dW [in, r]

    @staticmethod
    def forward(ctx, arith, x0, *params):
        x0 = x0.contiguous()
        L = len(params) // 3
        M, n_in = x0.shape
        ctx.bf16 = LowRankCrossNetFunction._bf16_ok(arith, M, n_in, params[0].size(0))
        if ctx.bf16:
            xl, xl16 = x0, ops.cast_bf16(x0, n_in, category="linear_fwd")
            xs16, vs16, us = [], [], []
            for l in range(L):
                V, W, b = params[3 * l], params[3 * l + 1], params[3 * l + 2]
                v16 = torch.empty((M, V.size(0)), dtype=torch.bfloat16, device=x0.device)
                ops.gemm_bf16(xl16, ops.cast_bf16(V, n_in, category="linear_fwd"), None, ACT_NONE, None, v16, category="linear_fwd")
                W16 = ops.cast_bf16(W, V.size(0), category="linear_fwd")
                xs16.append(xl16); vs16.append(v16)
                # x_{l+1} = x0 * (v W^T + b) + x_l inside the GEMM's epilogue (DLRM_CROSS_FUSE=0: the two kernels of round 4): the fp32 u
                # never goes through HBM, its bf16 copy is all the backward pass reads
                fused = ops.gemm_bf16_cross(v16, W16, b, x0, xl, want16=(l + 1 < L)) if CROSS_FUSE else None
                if fused is not None:
                    xl, xl16, u = fused
                    us.append(u)
                    continue
                u = torch.empty((M, n_in), dtype=torch.float32, device=x0.device)
                ops.gemm_bf16(v16, W16, b, ACT_NONE, u, None, category="linear_fwd")
                us.append(u)
                if l + 1 < L:
                    xl, xl16 = ops.cross_fwd(x0, u, xl, want16=True)
                else:
                    xl = ops.cross_fwd(x0, u, xl)
            ctx.arith, ctx.L = arith, L
            ctx.save_for_backward(*params, x0, *xs16, *vs16, *us)
            return xl
        xs, vs, us = [x0], [], []
        for l in range(L):
            V, W, b = params[3 * l], params[3 * l + 1], params[3 * l + 2]
            v = alloc2d(M, V.size(0), x0)
            ops.linear_fwd(xs[-1], V, None, ACT_NONE, v, arith)
            u = torch.empty((M, n_in), dtype=torch.float32, device=x0.device)
            ops.linear_fwd(v, W, b, ACT_NONE, u, arith)
            xs.append(ops.cross_fwd(x0, u, xs[-1]))
            vs.append(v); us.append(u)
        ctx.arith, ctx.L = arith, L
        ctx.save_for_backward(*params, *xs[:-1], *vs, *us)
        return xs[-1]

    @staticmethod
    def backward(ctx, g):
        L, arith = ctx.L, ctx.arith
        sv = ctx.saved_tensors
        if ctx.bf16:
            params, x0 = sv[:3 * L], sv[3 * L]
            xs16, vs16, us = sv[3 * L + 1:4 * L + 1], sv[4 * L + 1:5 * L + 1], sv[5 * L + 1:6 * L + 1]
            M, n_in = x0.shape
            g = g.contiguous()
            dx0 = torch.empty_like(x0)
            grads = [None] * (3 * L)
            gsum = None                                                               # g + sum of the V-path gradients so far (own buffer)
            for l in range(L - 1, -1, -1):
                V, W = params[3 * l], params[3 * l + 1]
                r = V.size(0)
                gl = g if gsum is None else gsum
                du16 = ops.cross_bwd(gl, x0, us[l], dx0, accumulate=(l != L - 1), out="bf16")   # du = g * x0 (bf16 only);  dx0 (+)= g * u_l
                dW, db = torch.empty_like(W), torch.empty(W.size(0), dtype=torch.float32, device=g.device)
                ops.linear_bwd_weight_bf16(du16, vs16[l], dW, db)
                dv16 = torch.empty((M, r), dtype=torch.bfloat16, device=g.device)
                ops.gemm_bf16(du16, ops.cast_bf16_transposed(W, n_in, category="linear_bwd_data"), None, ACT_NONE, None, dv16,
                              category="linear_bwd_data")
                dV = torch.empty_like(V)
                ops.linear_bwd_weight_bf16(dv16, xs16[l], dV, None)
                # gradient reaching x_l = identity path + V path: g + dv . V, summed in the GEMM epilogue (the incoming g itself is never
                # written: the first layer processed gets a fresh buffer, later ones accumulate in place)
                # (layer 0: x_l IS x_0, so the accumulated Hadamard-path gradient dx0 joins the same epilogue: dx0 + g + dv . V, in place)
                out = dx0 if l == 0 else (torch.empty_like(x0) if gsum is None else gsum)
                ops.gemm_bf16(dv16, ops.cast_bf16_transposed(V, r, category="linear_bwd_data"), None, ACT_NONE, out, None,
                              category="linear_bwd_data", addend=gl, addend2=dx0 if l == 0 else None)
                gsum = out
                grads[3 * l], grads[3 * l + 1], grads[3 * l + 2] = dV, dW, db
            return (None, gsum, *grads)
        params, xs, vs, us = sv[:3 * L], sv[3 * L:4 * L], sv[4 * L:5 * L], sv[5 * L:6 * L]
        x0 = xs[0]
        M, n_in = x0.shape
        g = g.contiguous()
        dx0 = torch.empty_like(x0)
        grads = [None] * (3 * L)
        for l in range(L - 1, -1, -1):
            V, W = params[3 * l], params[3 * l + 1]
            du = ops.cross_bwd(g, x0, us[l], dx0, accumulate=(l != L - 1))        # du = g * x0;  dx0 (+)= g * u_l
            dW, db = torch.empty_like(W), torch.empty(W.size(0), dtype=torch.float32, device=g.device)
            ops.linear_bwd_weight(du, vs[l], dW, db, arith=arith)
            dv = alloc2d(M, V.size(0), x0)
            ops.linear_bwd_data(du, W, None, ACT_NONE, dv, arith)
            dV = torch.empty_like(V)
            ops.linear_bwd_weight(dv, xs[l], dV, None, arith=arith)
            dxl = torch.empty_like(x0)
            ops.linear_bwd_data(dv, V, None, ACT_NONE, dxl, arith)
            g = ops.add(g, dxl)                                                   # gradient reaching x_l: identity path + V path
            grads[3 * l], grads[3 * l + 1], grads[3 * l + 2] = dV, dW, db
        dx0 = ops.add(dx0, g)                                                     # x_l of layer 0 IS x_0
        return (None, dx0, *grads)


class ChunkPackFunction(Function):
    """Re-orders the rows of the pooled-embedding send buffer for a PIPELINED all-to-all.

    `E` is [B, W] in global-batch order (rank r's samples are rows r*Bl .. (r+1)*Bl, Bl = B/N).  Chunk c of the pipeline
    holds, for every destination rank r, the c-th sub-slice (Bc = Bl/C rows) of r's samples; the function returns C tensors
    [N*Bc, W] (views of one [C, N, Bc, W] buffer), each of which is a complete, smaller all-to-all send buffer.  Backward
    scatters the C gradient buffers back to global-batch order for the fused embedding update."""

    @staticmethod
    def forward(ctx, E, N, C):
        B, W = E.shape
        Bc = B // (N * C)
        if Bc * N * C != B:
            raise RuntimeError("dlrm_amd: batch %d does not split into %d ranks x %d chunks" % (B, N, C))
        packed = _rowmajor(E).reshape(N, C, Bc, W).permute(1, 0, 2, 3).contiguous()
        ctx.dims = (N, C, Bc, W)
        return tuple(packed[c].view(N * Bc, W) for c in range(C))

    @staticmethod
    def backward(ctx, *grads):
        N, C, Bc, W = ctx.dims
        dE = torch.empty((N, C, Bc, W), dtype=grads[0].dtype, device=grads[0].device)
        for c, g in enumerate(grads):
            dE[:, c].copy_(g.reshape(N, Bc, W))
        return dE.view(N * C * Bc, W), None, None


class CatFunction(Function):
    """R = torch.cat(blocks, dim=1) — the "cat" interaction (dlrm_s_pytorch.py:505-507).

    forward(shared, block0, block1, ...): `shared` is None (R is allocated and filled by ONE strided-copy launch), or an
    OutSlot over a buffer in which the blocks ALREADY sit side by side in order (the [B, (1+T)*D] feature buffer the
    bottom tower and the embedding kernel wrote into): then R is that buffer and nothing is copied.  Backward hands out
    column views of dR (consumers take row strides)."""

    @staticmethod
    def forward(ctx, shared, *blocks):
        ctx.widths = [b.size(1) for b in blocks]
        if shared is not None:
            R = shared.get()
            if R.size(1) != sum(ctx.widths):
                raise RuntimeError("dlrm_amd: CatFunction shared buffer width mismatch")
            return R
        blocks = [_rowmajor(b) for b in blocks]
        R = alloc2d(blocks[0].size(0), sum(ctx.widths), blocks[0])
        dsts, o = [], 0
        for w in ctx.widths:
            dsts.append(R[:, o:o + w])
            o += w
        ops.copy_blocks(blocks, dsts)
        return R

    @staticmethod
    def backward(ctx, dR):
        outs, o = [], 0
        for w in ctx.widths:
            outs.append(dR[:, o:o + w])
            o += w
        return (None, *outs)


class ClampFunction(Function):
    """torch.clamp(p, lo, hi) of the predictions (--loss-threshold, dlrm_s_pytorch.py:580-583,607-610)."""

    @staticmethod
    def forward(ctx, p, lo, hi):
        p = p.contiguous()
        ctx.save_for_backward(p)
        ctx.lo, ctx.hi = lo, hi
        return ops.clamp(p, lo, hi)

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return ops.clamp_bwd(p, ctx.lo, ctx.hi, g), None, None


class BCELossFunction(Function):
    """BCELoss(reduction='mean'); loss and dL/dp are produced by one kernel pass.  class_weights = (w_neg, w_pos) turns it
    into the reference's weighted BCE (mean of loss_ws[T.long()] * bce, loss_fn_wrap dlrm_s_pytorch.py:150-156)."""

    @staticmethod
    def forward(ctx, p, target, weights, class_weights=(1.0, 1.0)):
        loss, dp = ops.bce_loss(p.contiguous(), target.contiguous(), weights, 1.0, want_grad=True, class_weights=class_weights)
        ctx.save_for_backward(dp)
        ctx.shape = p.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return ops.scale_by_scalar(dp, g.reshape(1).float()).view(ctx.shape), None, None, None


class BCEWithLogitsLossFunction(Function):
    """BCEWithLogitsLoss(reduction='mean') on raw logits (torchrec DLRMTrain); loss and dL/dlogits in one kernel pass."""

    @staticmethod
    def forward(ctx, z, target):
        loss, dz = ops.bce_logits_loss(z.contiguous(), target.contiguous(), 1.0, want_grad=True)
        ctx.save_for_backward(dz)
        ctx.shape = z.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return ops.scale_by_scalar(dz, g.reshape(1).float()).view(ctx.shape), None


class BCEElementwiseFunction(Function):
    """BCELoss(reduction='none'): the per-sample loss the reference's wbce path multiplies by class weights and averages
    in loss_fn_wrap (dlrm_s_pytorch.py:388-391, 150-156)."""

    @staticmethod
    def forward(ctx, p, target):
        p, target = p.contiguous(), target.contiguous()
        ctx.save_for_backward(p, target)
        return ops.bce_elementwise(p, target)

    @staticmethod
    def backward(ctx, g):
        p, target = ctx.saved_tensors
        return ops.bce_elementwise_bwd(p, target, g.to(torch.float32)), None


class MSELossFunction(Function):
    @staticmethod
    def forward(ctx, p, target):
        loss, dp = ops.mse_loss(p.contiguous(), target.contiguous(), 1.0, want_grad=True)
        ctx.save_for_backward(dp)
        ctx.shape = p.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return ops.scale_by_scalar(dp, g.reshape(1).float()).view(ctx.shape), None
