"""DLRM_Net for MI355X: the module surface of the reference's `DLRM_Net`
(dlrm_s_pytorch.py:207-612), every device operation a hand-written HIP kernel.

Drop-in contract:
  * constructor signature, `forward(dense_x, lS_o, lS_i)`, the public helpers `create_mlp`,
    `create_emb`, `apply_mlp`, `apply_emb`, `interact_features`, and the attributes
    `emb_l / v_W_l / bot_l / top_l / loss_fn / loss_ws / ndevices / loss_threshold /
    weighted_pooling / quantize_emb`;
  * `state_dict()` keys and shapes: `emb_l.{k}.weight`, `bot_l.{2i}.weight|bias`, `top_l.{2i}...`;
  * parameter initialisation consumes the numpy RNG in the reference's order (tables, bottom tower,
    top tower; weight then bias), so equal seeds give equal initial parameters;
  * `ext_dist.my_size > 1` selects the table-sharded / batch-split distributed forward;
  * configuration errors terminate through `sys.exit("ERROR: ...")` like the reference.
What differs by design: embedding parameters never receive a `.grad`; their sparse update is fused
into one kernel that runs when the optimizer steps (see `EmbeddingUpdateHook`), so the COO gradient
of the reference (nnz x D floats per table) is never written to HBM.
"""
from __future__ import annotations

import contextlib
import os
import sys
import weakref
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import ext_dist, ops
from .functional import (BCEElementwiseFunction, BCELossFunction, CatFunction, ChunkPackFunction, ClampFunction,
                         EmbeddingBagsFunction, GatherInteractFunction, InteractFunction, MLPFunction, MSELossFunction,
                         MDEmbeddingBagsFunction, OutSlot, QREmbeddingBagsFunction)
from . import functional as _functional
from .functional import MLP_CONSUMER_APPLIES_LAST_ACT, _side_stream

# one-lookup-per-bag verdict of untagged offsets: left on the device as a launch predicate (default) or waited for by the host (0)
DEVICE_PREDICATE = os.environ.get("DLRM_DEVICE_PREDICATE", "1") != "0"
from .ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, BagBatch

# Default of DLRM_Net.fuse_quant_interact.  Rule: True only if the fused quantised forward kernel is faster than dlrm_emb_fwd_quant +
# dlrm_interact_fwd at Criteo-Terabyte shapes at BOTH 4 and 8 bits, measured in one process (tools/bench_quant_interact.py;
# profiles/quant_emb/fused_interact_rates.md holds the table that decided it).
# Measured: 0.239 ms fused / 0.513 ms two kernels at 8 bits, 0.247 / 0.498 ms at 4 bits.
FUSE_QUANT_INTERACT_DEFAULT = True


_EMB_INIT_DEVICE = None


def set_embedding_init(device=None) -> None:
    """None (default): tables are drawn from numpy's global RNG exactly like the reference
    (dlrm_s_pytorch.py:280-284).  A torch device: tables are allocated and drawn U(-sqrt(1/n), sqrt(1/n))
    directly in that device's memory (needed for the 96 GB Criteo-Terabyte tables)."""
    global _EMB_INIT_DEVICE
    _EMB_INIT_DEVICE = device


_EMB_DTYPE = None           # None: fp32 tables; (torch.bfloat16, rounding, seed): set_embedding_dtype


def set_embedding_dtype(dtype=None, rounding: str = "stochastic", seed: int = 0) -> None:
    """None / torch.float32 (default): fp32 tables.  torch.bfloat16: every DLRM_Net built from here on creates its tables in bfloat16
    (DLRM_Net.embedding_bfloat16 applied at construction: each table is drawn in fp32 and converted before the next one is drawn, so the
    peak is the bf16 tables plus one fp32 table) with the given update rounding ("stochastic" | "nearest") and seed."""
    global _EMB_DTYPE
    if dtype is None or dtype == torch.float32:
        _EMB_DTYPE = None
        return
    if dtype != torch.bfloat16:
        sys.exit("ERROR: embedding tables are float32 or bfloat16, got " + str(dtype))
    if rounding not in ops.BF16_ROUNDINGS:
        sys.exit("ERROR: bfloat16 embedding tables round 'stochastic' or 'nearest', got " + repr(rounding))
    _EMB_DTYPE = (torch.bfloat16, rounding, int(seed))


class FusedRoute(NamedTuple):
    """one row of fused_route's table"""
    kind: str               # a key of ops.ROW_KINDS and functional.GATHER_KINDS; "fp32": dlrm_interact_*_gather
    none_fused: bool        # undecided offsets (a HIP graph is being captured) run the fused kernels alone; False: the two-kernel form
    host_proof: bool        # DLRM_DEVICE_PREDICATE=0 makes the host wait for the offsets' verdict; False: always the device-side state
    align: int              # bytes every table's base address must be a multiple of (one lane's load of a row)
    presort: bool           # the backward may take the SGD step of single-lookup rows itself (bags.presort)
    autograd: bool          # False: a forward-only kernel, no autograd node (packed tables)


# tables -> (route of D = 16 / 32 / 64, its ops.*_ok; route of D = 128, its ops.*_ok).  Given (tables, D) at most one of the two *_ok answers
# is true — every D = 128 one requires D == 128, every narrow one is dlrm_interact_gather_narrow_ok — and every table kind has its own row:
# the routes exclude each other.
_ROUTES = {
    "quant": ("narrow_quant", "gather_narrow_quant_ok", "quant", "gather_quant_ok"),
    "qr": ("narrow_qr", "gather_narrow_qr_ok", "qr", "gather_qr_ok"),
    "bf16": ("narrow_bf16", "gather_narrow_bf16_ok", "bf16", "gather_bf16_ok"),
    "fp32": ("narrow", "gather_narrow_ok", "fp32", "gather_ok"),
}


def fused_route(tables: str, F: int, D: int, bits: int = 0, *, fuse_emb_interact: bool, fuse_quant_interact: bool, fuse_qr_interact: bool,
                fuse_bf16_interact: bool, fuse_narrow_interact: bool, update_in_backward: bool, interaction_op: str = "dot",
                on_gpu: bool = True, pooling_weights: bool = False, grad_wanted: bool = False, bf16_rows: bool = False) -> Optional[FusedRoute]:
    """Which fused lookup + interaction kernels a model runs, decided once and from plain values: None = the two-kernel form.
    tables: "fp32" | "bf16" | "qr" | "md" | "quant" (packed; `bits` 4 | 8); F = 1 + T features of width D; the model's fuse_* attributes and
    update_in_backward; grad_wanted (packed tables only): the forward wants a gradient through the bottom tower, which only InteractFunction
    carries; bf16_rows: a QR list stored as bfloat16 (no kernel).  Touches no device and allocates nothing: the ops.gather_*_ok asked only
    load the library.  What a batch has to add at run time — B lookups per table, aligned tables, the offsets' state — is asked by
    DLRM_Net._fused_forward, after the route.

    Common to every route: fuse_emb_interact, the dot interaction, a GPU batch, no mixed-dimension table, no pooling weights.  Then
      tables   admitted by                              D = 16 / 32 / 64 with fuse_narrow_interact   else D = 128
      quant    fuse_quant_interact, no grad_wanted      narrow_quant                                 quant
      qr       fuse_qr_interact, no bf16_rows           narrow_qr                                    qr
      bf16     fuse_bf16_interact                       narrow_bf16                                  bf16
      fp32     (always)                                 narrow                                       fp32, presort iff update_in_backward
    The narrow routes of trained tables keep the two-kernel form for undecided offsets (none_fused False); the packed routes have no autograd
    node and never wait for a host-side proof; align is ops.RowKind.align of the kind, ops.packed_align(bits), or ops.GATHER_ALIGN."""
    if not (fuse_emb_interact and interaction_op == "dot" and on_gpu) or tables == "md" or pooling_weights:
        return None
    packed = tables == "quant"
    shape = (F, D, bits) if packed else (F, D)
    if packed:
        own = fuse_quant_interact and not grad_wanted
    elif tables == "qr":
        own = fuse_qr_interact and not bf16_rows
    else:
        own = fuse_bf16_interact if tables == "bf16" else True
    if not own:
        return None
    narrow, narrow_ok, wide, wide_ok = _ROUTES[tables]
    if fuse_narrow_interact and getattr(ops, narrow_ok)(*shape):
        kind = narrow
    elif getattr(ops, wide_ok)(*shape):
        kind = wide
    else:
        return None
    align = ops.packed_align(bits) if packed else ops.GATHER_ALIGN if kind == "fp32" else ops.ROW_KINDS[kind].align
    return FusedRoute(kind, packed or kind == wide, not packed, align, kind == "fp32" and bool(update_in_backward), not packed)


def _mix_seed(seed: int, call_no: int, stream_id: int = 0) -> int:
    """distinct Philox keys per (model seed, update call): the mix of datagen.UniformBatchGenerator._seed"""
    z = (seed * 0x9E3779B97F4A7C15 + call_no * 0xBF58476D1CE4E5B9 + stream_id * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    return z & (2 ** 64 - 1)


class FusedMLP(nn.Sequential):
    """nn.Sequential of Linear / ReLU / Sigmoid children (same child names -> same state_dict keys as
    the reference tower) whose forward runs the whole tower through the fused GEMM kernels.
    Being an nn.Module it can be wrapped by DistributedDataParallel exactly like the reference's.

    `arith` ("f32" default | "bf16x6" | "bf16", see ops.arith_code) is the arithmetic of this tower's GEMMs; it is a
    property of the module and is handed to every C-ABI call — there is no process-wide switch."""

    arith = os.environ.get("DLRM_MLP_ARITH", "f32")
    quant_bits = 32            # 8 / 16 after quantize(): an inference tower (see quantize)

    def _layers(self):
        mods = list(self.children())
        params, acts = [], []
        i = 0
        while i < len(mods):
            lin = mods[i]
            if not isinstance(lin, nn.Linear):
                raise RuntimeError("FusedMLP expects Linear layers each followed by ReLU or Sigmoid")
            act = ACT_NONE
            if i + 1 < len(mods) and isinstance(mods[i + 1], (nn.ReLU, nn.Sigmoid)):
                act = ACT_RELU if isinstance(mods[i + 1], nn.ReLU) else ACT_SIGMOID
                i += 1
            params += [lin.weight, lin.bias]
            acts.append(act)
            i += 1
        return params, tuple(acts)

    def forward(self, x, out_slot: Optional[OutSlot] = None, consumer_applies_last_act: bool = False):
        """consumer_applies_last_act: the caller promises that the ONLY consumer of the output multiplies the gradient it sends back
        by the derivative of this tower's last ReLU (the interaction backward kernels do, ops.INTERACT_RELU_X) — the tower's
        backward then skips that pass.  Ignored (False) for towers that do not end in a ReLU."""
        if self.quant_bits != 32:
            return self._forward_quantized(x, out_slot)
        params, acts = self._layers()
        flag = MLP_CONSUMER_APPLIES_LAST_ACT if (consumer_applies_last_act and acts and acts[-1] == ACT_RELU) else 0
        return MLPFunction.apply(x, acts, out_slot, ops.arith_code(self.arith) | flag, *params)

    def quantize(self, bits):
        """torch.quantization.quantize_dynamic(tower, {nn.Linear}, qint8 | float16) on the device (dlrm_s_pytorch.py:1473-1480).
        8: every Linear's weight is packed once as torch packs it (per tensor, symmetric: ops.q8_pack_weight) and forward runs, per layer,
        the per-call activation quantisation and the int8 MFMA GEMM (ops.linear_q8).  16: the weights are rounded through fp16 in place
        (saturating at 65504 like torch's packing) and stay fp32 operands of the fp32 GEMM path; activations stay fp32 as in the reference.
        Any other value returns without change.  From here on the tower is an inference tower: its forward carries no autograd node.
        The packed int8 weights are not parameters, buffers or state_dict entries (the state_dict keeps the reference's keys and the fp32
        weights stay, so an int8 tower holds 1.25x the weight bytes, not less): `.to()` / `.cuda()` / `.half()` would leave them behind and
        `load_state_dict` would change weights that forward no longer reads (or, at 16 bits, store unrounded ones), so both are refused."""
        if bits not in (8, 16):
            return
        if self.quant_bits != 32:
            sys.exit("ERROR: the MLP tower is quantized already (%d bits)" % self.quant_bits)
        params, acts = self._layers()
        if not params or any(not p.is_cuda for p in params):
            raise RuntimeError("dlrm_amd: quantize packs the tower's weights on the GPU and the quantized layers have no CPU path; "
                               "move the model to the device first (model.to('cuda'))")
        if bits == 8:
            self._q8 = [ops.q8_pack_weight(params[2 * i].detach()) for i in range(len(acts))]
        else:
            with torch.no_grad():
                for i in range(len(acts)):
                    W = params[2 * i]
                    W.copy_(W.clamp(-65504.0, 65504.0).half().float())
        self.quant_bits = bits

    def _apply(self, fn, *args, **kwargs):
        if self.quant_bits != 32:
            sys.exit("ERROR: a quantized MLP tower (%d bits) cannot be moved or converted (.to / .cuda / .cpu / .half): its packed weights "
                     "live on the device they were packed on" % self.quant_bits)
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        if self.quant_bits != 32:
            sys.exit("ERROR: load_state_dict into a quantized MLP tower (%d bits): quantized towers are constants (inference only) — load "
                     "the fp32 weights first, then quantize" % self.quant_bits)
        return super()._load_from_state_dict(*args, **kwargs)

    def _forward_quantized(self, x, out_slot: Optional[OutSlot]):
        params, acts = self._layers()
        with torch.no_grad():
            if self.quant_bits == 16:
                return MLPFunction.apply(x.detach(), acts, out_slot, ops.arith_code("f32"), *[p.detach() for p in params])
            cur = x.detach()
            if cur.dim() != 2 or (cur.numel() and cur.stride(1) != 1):
                cur = cur.contiguous()
            L = len(acts)
            for i in range(L):
                out = out_slot.get() if (i == L - 1 and out_slot is not None) else None
                cur = ops.linear_q8(cur, self._q8[i], params[2 * i + 1].detach(), acts[i], out)
            return cur

    def ends_in_relu(self) -> bool:
        mods = list(self.children())
        return bool(mods) and isinstance(mods[-1], nn.ReLU)


class FusedBCELoss(nn.Module):
    """BCELoss(reduction="mean") computed by the fused loss kernel."""

    def forward(self, p, target):
        return BCELossFunction.apply(p, target, None)


class FusedBCELossNone(nn.Module):
    """BCELoss(reduction="none") by the elementwise loss kernel: what `loss_fn` is under --loss-function=wbce, where the
    reference's loss_fn_wrap multiplies it by loss_ws[T] and takes the mean (dlrm_s_pytorch.py:150-156)."""

    def forward(self, p, target):
        return BCEElementwiseFunction.apply(p, target)


class FusedMSELoss(nn.Module):
    def forward(self, p, target):
        return MSELossFunction.apply(p, target)


class QREmbeddingBagHolder(nn.Module):
    """Parameter holder of one quotient-remainder table (the reference's tricks/qr_embedding_bag.py QREmbeddingBag, mode="sum", sparse):
    `weight_q` [ceil(n / c), D] and `weight_r` [c, D], so that state_dict has the reference's keys `emb_l.{k}.weight_q|weight_r`, plus the
    reference's constants.  Both are drawn U(sqrt(1 / n), 1) from TORCH's generator, q then r: the reference calls
    `nn.init.uniform_(w, np.sqrt(1 / n))`, whose second positional argument is the LOWER bound (the upper one stays 1.0) — restated
    exactly, because equal seeds must give equal initial parameters.  Lookups of a model go through dlrm_emb_fwd_qr for all tables at once
    (QREmbeddingBagsFunction) and are trained through the model's gradient sink; `forward` here is the same kernel for this table alone and is
    FORWARD-ONLY: its result carries no autograd node (a holder on its own has no sink for the sparse gradients)."""

    def __init__(self, num_categories: int, embedding_dim: int, num_collisions: int, operation: str = "mult", device=None):
        super().__init__()
        self.num_categories, self.num_collisions, self.operation = int(num_categories), int(num_collisions), operation
        self.embedding_dim = [int(embedding_dim), int(embedding_dim)]
        self.num_embeddings = [ops.qr_rows_q(num_categories, num_collisions), int(num_collisions)]
        self.mode, self.sparse = "sum", True
        low = float(np.sqrt(1 / num_categories))
        self.weight_q = nn.Parameter(torch.empty((self.num_embeddings[0], embedding_dim), dtype=torch.float32, device=device))
        self.weight_r = nn.Parameter(torch.empty((self.num_embeddings[1], embedding_dim), dtype=torch.float32, device=device))
        with torch.no_grad():
            self.weight_q.uniform_(low, 1.0)
            self.weight_r.uniform_(low, 1.0)

    def forward(self, input, offsets=None, per_sample_weights=None):
        if per_sample_weights is not None:
            sys.exit("ERROR: quotient remainder with weighted pooling is not supported")
        if offsets is None:
            raise RuntimeError("dlrm_amd: QREmbeddingBagHolder takes 1-D indices with bag offsets")
        spec = ([self.num_categories], [self.num_collisions], self.operation, False)      # (no pooled sums kept: nothing flows back)
        with torch.no_grad():
            return QREmbeddingBagsFunction.apply(None, ops.BagBatch([offsets], [input]), None, spec, self.weight_q, self.weight_r)

    def extra_repr(self):
        return "%d, %d, collisions=%d, operation=%s" % (self.num_categories, self.embedding_dim[0], self.num_collisions, self.operation)


class PrEmbeddingBagHolder(nn.Module):
    """Parameter holder of one mixed-dimension table (the reference's tricks/md_embedding_bag.py PrEmbeddingBag): `embs`, an
    nn.EmbeddingBag(n, d, mode="sum", sparse=True) holder, and `proj`, nn.Linear(d, base, bias=False) when d < base and nn.Identity() when
    equal — state_dict has the reference's keys `emb_l.{k}.embs.weight` and `emb_l.{k}.proj.weight`.  On the CPU (device None) it is built by
    the reference's own calls in the reference's order, because equal seeds must give equal initial parameters: nn.EmbeddingBag's N(0, 1)
    init and xavier_uniform_ on the table (both replaced below, both spend torch's generator), nn.Linear's init and xavier_uniform_ on the
    projection, then the table from numpy's U(-sqrt(1/n), sqrt(1/n)) (dlrm_s_pytorch.py:270-275).  With a device the table is drawn there
    from the same distribution (no parity claim).  Lookups of a model go through dlrm_emb_fwd_md for all tables at once
    (MDEmbeddingBagsFunction); `forward` here is the same kernel for this table alone and is FORWARD-ONLY, like the QR holder's."""

    def __init__(self, num_embeddings: int, embedding_dim: int, base_dim: int, device=None):
        super().__init__()
        n, d, base = int(num_embeddings), int(embedding_dim), int(base_dim)
        if d > base:
            raise ValueError("Embedding dim " + str(d) + " > base dim " + str(base))
        self.base_dim = base
        bound = np.sqrt(1 / n)
        if device is None:
            self.embs = nn.EmbeddingBag(n, d, mode="sum", sparse=True)
            torch.nn.init.xavier_uniform_(self.embs.weight)
        if d < base:
            self.proj = nn.Linear(d, base, bias=False)
            torch.nn.init.xavier_uniform_(self.proj.weight)
        else:
            self.proj = nn.Identity()
        if device is None:
            w = np.random.uniform(low=-bound, high=bound, size=(n, d)).astype(np.float32)
            self.embs.weight.data = torch.tensor(w, requires_grad=True)
        else:
            w = torch.empty((n, d), dtype=torch.float32, device=device).uniform_(-bound, bound)
            self.embs = nn.EmbeddingBag(n, d, mode="sum", sparse=True, _weight=w)

    def proj_weight(self):
        return self.proj.weight if isinstance(self.proj, nn.Linear) else None

    def forward(self, input, offsets=None, per_sample_weights=None):
        if per_sample_weights is not None:
            sys.exit("ERROR: mixed dimensions with weighted pooling is not supported")
        if offsets is None:
            raise RuntimeError("dlrm_amd: PrEmbeddingBagHolder takes 1-D indices with bag offsets")
        p = self.proj_weight()
        spec = (self.base_dim, [p is not None], False)       # (no pooled sums kept: nothing flows back)
        with torch.no_grad():
            return MDEmbeddingBagsFunction.apply(None, ops.BagBatch([offsets], [input]), None, spec, self.embs.weight, *([p] if p is not None else []))


class EmbeddingUpdateHook:
    """Applies the fused sparse embedding update when an optimizer steps.

    `run()` in the reference builds `torch.optim.SGD(dlrm.parameters())` and calls
    zero_grad / backward / step (dlrm_s_pytorch.py:1343-1369, 1611-1621).  Embedding parameters keep
    `.grad is None` (SGD skips them); backward parks (weights, bags, d_out) here and a global
    optimizer step pre-hook launches `dlrm_emb_bwd_sgd` with the learning rate the optimizer holds at
    that moment — the same point in the step, with the same lr, as the reference's sparse update."""

    _models: "weakref.WeakSet" = weakref.WeakSet()
    _handle = None
    _post = None

    @classmethod
    def register(cls, model: "DLRM_Net") -> None:
        cls._models.add(model)
        if cls._handle is None:
            from torch.optim.optimizer import register_optimizer_step_post_hook, register_optimizer_step_pre_hook
            cls._handle = register_optimizer_step_pre_hook(cls._pre_step)
            cls._post = register_optimizer_step_post_hook(cls._post_step)

    @staticmethod
    def _pre_step(optimizer, args, kwargs):
        for model in list(EmbeddingUpdateHook._models):
            if getattr(model, "quantize_mlp_bits", 32) != 32:
                model._refuse_step_if_mlp_quantized(optimizer)
            if getattr(model, "quantize_emb", False):
                model._refuse_step_if_quantized(optimizer)
                continue
            if (model.overlap_streams or model.update_in_backward) and model._bound_optimizer is None and model._owned_by(optimizer):
                model._bound_optimizer = weakref.ref(optimizer)      # (what lets the NEXT backward pass launch / take the sparse update itself)
            if model._pending_emb:
                model.apply_pending_embedding_updates(optimizer)

    @staticmethod
    def _post_step(optimizer, args, kwargs):
        # overlap mode: the embedding update runs on the side stream; once optimizer.step() has returned, everything the
        # caller enqueues on ITS stream (state_dict reads, evaluation, the next forward) is ordered after it
        for model in list(EmbeddingUpdateHook._models):
            model._join_side_stream()


class ParkedGrad(NamedTuple):
    """one backward pass of the embedding lookups, parked in DLRM_Net._pending_emb until an optimizer that owns the tables steps"""
    weights: Sequence[torch.Tensor]
    bags: BagBatch
    dout: torch.Tensor                          # the [B, >= T*D] gradient buffer of the pooled lookups
    presorted: Optional["ops.Presorted"] = None        # the backward pass already took the single-lookup rows (update_in_backward)


# (update, tables) -> why that update is not built for those tables; every other pair runs.  update: the head of an _embedding_update_plan
# result — "sgd", "rwsadagrad", "adagrad", "coo" — or "unfused" (fused_emb_update = False: the COO gradient whatever the optimizer);
# tables: DLRM_Net._table_kind().  Read by DLRM_Net._refuse_update alone.
UPDATE_REFUSALS = {
    ("adagrad", "bf16"): "ERROR: the fused exact Adagrad update is not built for bfloat16 embedding tables; use SGD or row-wise Adagrad",
    ("adagrad", "qr"): "ERROR: the fused exact Adagrad update is not built for QR embedding tables; use SGD, or set "
                       "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("adagrad", "md"): "ERROR: the fused exact Adagrad update is not built for mixed-dimension embedding tables; use SGD, or set "
                       "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("rwsadagrad", "qr"): "ERROR: the fused row-wise Adagrad update is not built for QR embedding tables; use SGD, or set "
                          "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("rwsadagrad", "md"): "ERROR: the fused row-wise Adagrad update is not built for mixed-dimension embedding tables; use SGD, or set "
                          "model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0) with a torch optimizer",
    ("coo", "bf16"): "ERROR: bfloat16 embedding tables are updated by the fused kernels only: plain SGD (no momentum, no weight "
                     "decay) or row-wise Adagrad; this optimizer needs the sparse COO gradient",
    ("unfused", "bf16"): "ERROR: bfloat16 embedding tables need the fused embedding update (fused_emb_update = False materialises sparse "
                         "fp32 COO gradients for a torch optimizer, which would round on every add)",
}


class DLRM_Net(nn.Module):
    # the torchrec variants set it False: their constructors take no qr_* argument, so the refusal in create_emb guards a subclass or a caller
    # that sets the qr_* attributes itself (ShardedDLRM calls create_emb directly)
    _qr_supported = True
    _md_supported = True        # (the same for mixed-dimension tables)
    _bf16_supported = True      # (the same for bfloat16 tables: embedding_bfloat16 / set_embedding_dtype)
    emb_bf16 = None             # (rounding, seed) once the tables are bfloat16
    # set by GraphedTrainStep(device_step_state=True): called in front of an EAGER bf16 key draw, so that _bf16_update_calls first takes in the
    # update calls the graph's replays made on the device (graph.py, "host mirrors")
    _step_state_settle = None
    # opt-in (launcher: --bf16-fuse-interact): a bfloat16 model enters the fused lookup + interaction branch of sequential_forward under the
    # fp32 branch's conditions and runs csrc/interact_bf16.hip (forward and backward) instead of dlrm_emb_fwd_bf16 + the interaction kernels
    # through the pooled [B, T*D] buffer — the same bits.  Off: a bfloat16 model runs exactly the two-kernel form.
    fuse_bf16_interact = False
    # opt-in (launcher: --qr-fuse-interact): a model with quotient-remainder tables enters the fused lookup + interaction branch of
    # sequential_forward under the fp32 branch's conditions and runs csrc/interact_qr.hip (forward and backward) instead of dlrm_emb_fwd_qr + the
    # interaction kernels + dlrm_emb_qr_bwd_split through the pooled [B, T*D] buffer and the [B, 2*Tq*D] pooled sums — the same bits.  Off: a QR
    # model runs exactly the two-kernel form.  D = 128; D = 16 / 32 / 64 (csrc/interact_narrow_qr.hip) only with fuse_narrow_interact set as well.
    fuse_qr_interact = False
    # opt-in (launcher: --narrow-fuse-interact): a model with plain fp32 tables of D = 16 / 32 / 64 enters the fused lookup + interaction branch
    # of sequential_forward under the fp32 branch's conditions and runs csrc/interact_narrow.hip (forward and backward) instead of dlrm_emb_fwd
    # + the generic interaction kernels through the pooled [B, T*D] buffer — the same bits.  Off: such a model runs exactly the two-kernel form.
    # Together with fuse_bf16_interact a bfloat16 model of those widths enters too (csrc/interact_narrow_rows.hip, forward and backward), and
    # together with fuse_quant_interact a quantised model of those widths takes the narrow fused forward of that file (fused_route),
    # and together with fuse_qr_interact a model with QR tables of those widths enters too (csrc/interact_narrow_qr.hip, forward and backward).
    fuse_narrow_interact = False
    # opt-in (launcher: --fused-adagrad): a stock torch.optim.Adagrad that owns the tables (the reference's --optimizer=adagrad) gets the fused
    # exact Adagrad update (csrc/adagrad.hip dlrm_emb_bwd_adagrad) on ITS state[p]["sum"], the step pre-hook advances the tables'
    # state[p]["step"], and the dense parameters stay with torch's own step.  Off: such an optimizer takes the sparse COO gradient, as before.
    # (dlrm_amd.optim.FusedAdagrad takes the fused update either way.)
    fused_adagrad = False
    quantize_mlp_bits = 32      # 8 / 16 after quantize_mlp()

    # ---------------------------------------------------------------- parameter construction
    def create_mlp(self, ln, sigmoid_layer):
        """Tower with ln[i] -> ln[i+1] Linear layers; Sigmoid after layer `sigmoid_layer`, ReLU after
        the others.  W ~ N(0, sqrt(2/(m+n))), b ~ N(0, sqrt(1/m)) drawn from numpy's global RNG
        (dlrm_s_pytorch.py:208-246)."""
        mods = []
        for i in range(ln.size - 1):
            fan_in, fan_out = int(ln[i]), int(ln[i + 1])
            lin = nn.Linear(fan_in, fan_out, bias=True)
            w = np.random.normal(0.0, np.sqrt(2 / (fan_out + fan_in)), size=(fan_out, fan_in)).astype(np.float32)
            b = np.random.normal(0.0, np.sqrt(1 / fan_out), size=fan_out).astype(np.float32)
            lin.weight.data = torch.tensor(w, requires_grad=True)
            lin.bias.data = torch.tensor(b, requires_grad=True)
            mods.append(lin)
            mods.append(nn.Sigmoid() if i == sigmoid_layer else nn.ReLU())
        return FusedMLP(*mods)

    def create_emb(self, m, ln, weighted_pooling=None):
        """One EmbeddingBag(sum) parameter holder per LOCAL table, W ~ U(-sqrt(1/n), sqrt(1/n)) from
        numpy's global RNG (dlrm_s_pytorch.py:248-294).  The holders own the parameters (state_dict
        parity); lookups go through the batched HIP kernel, not through the holders' forward."""
        tables = nn.ModuleList()
        pool_w = []
        if _EMB_DTYPE is not None:
            # tables created in bfloat16 (set_embedding_dtype): every refusal before a table is built
            self._refuse_bf16(weighted_pooling == "learned" or (weighted_pooling is not None and weighted_pooling != "fixed"),
                              bool(getattr(self, "qr_flag", False)), bool(getattr(self, "md_flag", False)))
        # --md-flag with per-table widths (dlrm_s_pytorch.py:1213-1219 turns m_spa into md_solver's list): every refusal before a table is built
        md = bool(getattr(self, "md_flag", False)) and not np.isscalar(m) and np.ndim(m) == 1
        m_plain, base = m, None
        if md:
            m = [int(d) for d in (m.tolist() if hasattr(m, "tolist") else m)]
            base = max(m)
            if len(m) != ln.size or min(m) < 1:
                sys.exit("ERROR: --md-flag needs one embedding dimension >= 1 per table, got %d for %d tables" % (len(m), ln.size))
            if not self._md_supported:
                sys.exit("ERROR: mixed-dimension embeddings are built for DLRM_Net only, not for the torchrec variants (%s)" % type(self).__name__)
            if weighted_pooling is not None:
                sys.exit("ERROR: mixed dimensions with weighted pooling is not supported")
            if getattr(self, "qr_flag", False):
                sys.exit("ERROR: --md-flag and --qr-flag cannot be combined (the reference builds QR tables only, with a list-valued dimension)")
            if ext_dist.is_distributed():
                sys.exit("ERROR: mixed-dimension embedding tables are single-process only (the table-sharded distributed forward is not "
                         "built for them)")
        for i in range(ln.size):
            if ext_dist.is_distributed() and i not in self.local_emb_indices:
                continue
            n = int(ln[i])
            if getattr(self, "qr_flag", False) and n > self.qr_threshold:
                # the reference's QREmbeddingBag (dlrm_s_pytorch.py:258-266): drawn from torch's generator, not numpy's (see the holder)
                if not self._qr_supported:
                    sys.exit("ERROR: QR embeddings are built for DLRM_Net only, not for the torchrec variants (%s)" % type(self).__name__)
                if weighted_pooling is not None:
                    sys.exit("ERROR: quotient remainder with weighted pooling is not supported")
                if self.qr_operation == "concat":
                    sys.exit("ERROR: --qr-operation=concat makes a QR table 2*D wide beside D-wide plain tables; the MI355X DLRM_Net keeps "
                             "every feature in one uniform [B, (1+T)*D] buffer, so only mult and add are supported")
                if self.qr_operation not in ops.QR_OPS:
                    sys.exit("ERROR: --qr-operation=" + str(self.qr_operation) + " is not supported")
                if int(self.qr_collisions) < 1:
                    sys.exit("ERROR: --qr-collisions must be at least 1 with --qr-flag, got " + str(self.qr_collisions))
                tables.append(QREmbeddingBagHolder(n, m, int(self.qr_collisions), self.qr_operation, device=_EMB_INIT_DEVICE))
                pool_w.append(None)
                continue
            if getattr(self, "md_flag", False) and n > self.md_threshold:
                if not md:
                    # (a scalar width with a table above the threshold: the reference raises TypeError at max(m) there)
                    sys.exit("ERROR: mixed-dimension embeddings are not supported by the MI355X DLRM_Net")
                # the reference's PrEmbeddingBag (dlrm_s_pytorch.py:267-275)
                tables.append(PrEmbeddingBagHolder(n, int(m[i]), base, device=_EMB_INIT_DEVICE))
                pool_w.append(None)
                continue
            if md:
                # a table at or below md_threshold: the reference hands the LIST m to nn.EmbeddingBag and raises; built here as the plain
                # [n, base] table its line 269 (`else base`) evidently meant — no reference counterpart
                m_plain = base
            bound = np.sqrt(1 / n)
            if getattr(self, "qr_flag", False) and _EMB_INIT_DEVICE is None:
                # the reference constructs nn.EmbeddingBag(n, m) first, whose own N(0, 1) init consumes n*m draws of TORCH's generator before
                # the numpy values replace it (dlrm_s_pytorch.py:277-284); the QR tables after this one are drawn from that generator, so
                # equal seeds give equal QR tables only if the same draws are spent here
                torch.empty((n, m_plain), dtype=torch.float32).normal_()
            if _EMB_INIT_DEVICE is None:
                w = torch.tensor(np.random.uniform(low=-bound, high=bound, size=(n, m_plain)).astype(np.float32))
            else:
                # benchmark-scale tables (tens of GB) cannot go through a float64 numpy temporary on the
                # host: same distribution, drawn on the device (see set_embedding_init)
                w = torch.empty((n, m_plain), dtype=torch.float32, device=_EMB_INIT_DEVICE).uniform_(-bound, bound)
            if _EMB_DTYPE is not None:
                w = w.to(torch.bfloat16)                 # round-to-nearest; the fp32 draw is released before the next table is drawn
            holder = nn.EmbeddingBag(n, m_plain, mode="sum", sparse=True, _weight=w)
            pool_w.append(None if weighted_pooling is None else torch.ones(n, dtype=torch.float32))
            tables.append(holder)
        return tables, pool_w

    def __init__(self, m_spa=None, ln_emb=None, ln_bot=None, ln_top=None, arch_interaction_op=None,
                 arch_interaction_itself=False, sigmoid_bot=-1, sigmoid_top=-1, sync_dense_params=True,
                 loss_threshold=0.0, ndevices=-1, qr_flag=False, qr_operation="mult", qr_collisions=0,
                 qr_threshold=200, md_flag=False, md_threshold=200, weighted_pooling=None,
                 loss_function="bce"):
        super().__init__()
        self._pending_emb: list = []
        self.emb_update_mode = ops.UPD_SORTED
        # False (or env DLRM_FUSED_EMB_UPDATE=0): backward materialises the reference's sparse COO gradient into
        # `emb.weight.grad` (dlrm_emb_bwd_coo) and ANY torch optimizer consumes it, exactly like the reference
        self.fused_emb_update = os.environ.get("DLRM_FUSED_EMB_UPDATE", "1") != "0"
        # True (or env DLRM_OVERLAP=1): the HBM-bound embedding kernels run on a second HIP stream beside the MFMA-bound MLP
        # GEMMs they do not depend on — forward: the pooled lookups beside the bottom MLP (the reference's own overlap idea,
        # dlrm_s_pytorch.py:563-568); backward: the fused sparse update beside the bottom-MLP backward and the dense
        # optimizer step.  Same kernels, same arithmetic, same results; optimizer.step() returns with the caller's stream
        # ordered after the update.
        self.overlap_streams = os.environ.get("DLRM_OVERLAP", "0") == "1"
        # Single-process forward with ONE lookup per bag (the Criteo data sets; DLRM_FUSE_EMB_INTERACT=0 turns it off), D = 128 and at most
        # 26 tables: the interaction kernels gather the embedding rows themselves (dlrm_interact_fwd_gather / _bwd_gather) and
        # apply_emb's pooled-embedding buffer is never written or re-read — bit-identical results, forward 0.21 ms instead of 0.34 +
        # 0.26 at Criteo-Terabyte shapes (profiles/round3).  Taken when every table has exactly B lookups AND the bag starts are proven
        # to be 0, 1, 2, ... (ops.offsets_are_iota, dlrm_amd/iota.py: one device pass + one synchronisation per distinct offsets tensor object, cached;
        # a ragged batch with nnz == B — an empty bag next to a two-lookup bag — takes the two kernels like every other multi-hot
        # input).  The kernels still verify the bag starts themselves and report a violation through the index-error block.
        self.fuse_emb_interact = os.environ.get("DLRM_FUSE_EMB_INTERACT", "1") == "1"
        # The same for a model whose tables are QUANTISED (quantize_embedding): one forward kernel fetches the packed rows, dequantises them
        # into its LDS image and multiplies (dlrm_interact_fwd_gather_quant) — the bits of dlrm_emb_fwd_quant + dlrm_interact_fwd without the
        # [B, T*D] fp32 buffer between them.  Taken under the conditions of fuse_emb_interact (which must be set too), when no gradient is
        # wanted from the forward.  Default: FUSE_QUANT_INTERACT_DEFAULT at the top of this file, decided by measurement.
        self.fuse_quant_interact = FUSE_QUANT_INTERACT_DEFAULT
        # True (or env DLRM_UPDATE_IN_BACKWARD=1; opt-in): once the model knows its plain-SGD optimizer (from that optimizer's first step), the
        # fused backward takes the SGD step of every embedding row that ONE lookup of the batch names — the row is staged in the interaction
        # kernel's LDS and its gradient is in registers, so the table row is written at once and neither the gradient row nor a second read of
        # the table row ever touches HBM (ABI 17: dlrm_emb_presort, dlrm_interact_bwd_gather_sgd, dlrm_emb_bwd_sgd_presorted; BASELINE
        # north_star "fused sparse SGD for the backward embedding update", torchrec's apply_optimizer_in_backward in dlrm_main.py).  Rows named
        # by several lookups are updated when the optimizer steps, as before.  After backward() + optimizer.step() the tables hold the bits the
        # step-time update writes (DLRM_UPD_SORTED); what differs is WHEN: single-lookup rows change during backward(), with the learning rate the
        # optimizer holds then (the reference loop changes it after step(): dlrm_s_pytorch.py:1620-1621).  A loop that calls backward() without
        # step(), or several times per step, must leave this off — as with overlap_streams, which moves the whole update into backward.
        self.update_in_backward = os.environ.get("DLRM_UPDATE_IN_BACKWARD", "0") == "1"
        self._bound_optimizer = None        # weakref to the optimizer that owns the tables (learnt at its first step)
        self._side_keep: list = []          # tensors the side stream still reads (released at the join)
        # > 1: the pooled-embedding all-to-all of the distributed forward is pipelined in that many batch chunks (opt-in)
        self.a2a_chunks = max(int(os.environ.get("DLRM_A2A_CHUNKS", "1")), 1)
        if m_spa is None or ln_emb is None or ln_bot is None or ln_top is None or arch_interaction_op is None:
            return  # empty shell, like the reference's guard (dlrm_s_pytorch.py:320-326)

        self.ndevices = ndevices
        self.output_d = 0
        self.parallel_model_batch_size = -1
        self.parallel_model_is_not_prepared = True
        self.arch_interaction_op = arch_interaction_op
        self.arch_interaction_itself = arch_interaction_itself
        self.sync_dense_params = sync_dense_params
        self.loss_threshold = loss_threshold
        self.loss_function = loss_function
        self.weighted_pooling = ("learned" if weighted_pooling is not None and weighted_pooling != "fixed"
                                 else weighted_pooling)
        self.qr_flag = qr_flag
        if qr_flag:
            self.qr_collisions, self.qr_operation, self.qr_threshold = qr_collisions, qr_operation, qr_threshold
        self.md_flag = md_flag
        if md_flag:
            self.md_threshold = md_threshold
        self.m_spa = m_spa

        if ext_dist.is_distributed():
            n_emb = len(ln_emb)
            if n_emb < ext_dist.my_size:
                sys.exit("only (%d) sparse features for (%d) devices, table partitions will fail"
                         % (n_emb, ext_dist.my_size))
            self.n_global_emb = n_emb
            self.n_local_emb, self.n_emb_per_rank = ext_dist.get_split_lengths(n_emb)
            self.local_emb_slice = ext_dist.get_my_slice(n_emb)
            self.local_emb_indices = list(range(n_emb))[self.local_emb_slice]

        if ndevices > 1:
            sys.exit("ERROR: single-process multi-GPU (ndevices=%d) is not supported; launch one process per "
                     "GPU (torchrun) to use table-sharded embeddings over RCCL" % ndevices)
        if md_flag and not np.isscalar(m_spa) and np.ndim(m_spa) == 1 and len(m_spa) and int(ln_bot[-1]) != int(max(m_spa)):
            # (run() checks the scalar before md_solver replaces it, dlrm_s_pytorch.py:1197-1219; the smallest table keeps it: base = max(m))
            sys.exit("ERROR: arch-sparse-feature-size " + str(int(max(m_spa))) + " does not match last dim of bottom mlp " + str(int(ln_bot[-1])))
        self.emb_l, pool_w = self.create_emb(m_spa, ln_emb, weighted_pooling)
        if _EMB_DTYPE is not None:
            self.emb_bf16 = (_EMB_DTYPE[1], _EMB_DTYPE[2])
            self._bf16_update_calls = 0
        if self.weighted_pooling == "learned":
            # dlrm_s_pytorch.py:370-375: the per-row pooling weights become parameters (state_dict keys v_W_l.{k})
            self.v_W_l = nn.ParameterList([nn.Parameter(w) for w in pool_w])
        else:
            self.v_W_l = pool_w
        self.bot_l = self.create_mlp(ln_bot, sigmoid_bot)
        self.top_l = self.create_mlp(ln_top, sigmoid_top)

        self.quantize_emb = False
        self.emb_l_q = []
        self.quantize_bits = 32

        if loss_function == "mse":
            self.loss_fn = FusedMSELoss()
        elif loss_function == "bce":
            self.loss_fn = FusedBCELoss()
        elif loss_function == "wbce":
            import __main__ as _m  # the reference reads the CLI global `args.loss_weights` (:391)
            lw = getattr(getattr(_m, "args", None), "loss_weights", "1.0-1.0")
            self.loss_ws = torch.tensor(np.fromstring(lw, dtype=float, sep="-"))
            self.loss_fn = FusedBCELossNone()
        else:
            sys.exit("ERROR: --loss-function=" + str(loss_function) + " is not supported")
        EmbeddingUpdateHook.register(self)

    def _interaction_mode(self) -> int:
        """0: strictly lower triangle, reference order (dlrm_s_pytorch.py:499-501); 1: with the diagonal (--arch-interaction-itself);
        2: torchrec's torch.triu_indices(F, F, 1) order (dlrm_amd.torchrec_variant)"""
        if getattr(self, "interaction_order", "tril") == "triu":
            if self.arch_interaction_itself:
                sys.exit("ERROR: the torchrec (triu) interaction order has no self-interaction")
            return 2
        return 1 if self.arch_interaction_itself else 0

    def set_mlp_arith(self, name: str) -> None:
        """Arithmetic of both towers' GEMMs (FusedMLP.arith): "f32" | "bf16x6" | "bf16"."""
        ops.arith_code(name)
        for tower in (self.bot_l, self.top_l):
            getattr(tower, "module", tower).arith = name        # DDP-wrapped towers keep the FusedMLP in .module

    # ---------------------------------------------------------------- operators
    def apply_mlp(self, x, layers, out_slot: Optional[OutSlot] = None, consumer_applies_last_act: bool = False):
        if consumer_applies_last_act:
            return layers(x, out_slot=out_slot, consumer_applies_last_act=True)
        if out_slot is not None:
            return layers(x, out_slot=out_slot)
        return layers(x)

    def _relu_x(self) -> int:
        """ops.INTERACT_RELU_X when the dot interaction's backward may apply the derivative of the bottom tower's last ReLU to its
        feature-0 gradient (and the tower is told to expect that: apply_mlp(..., consumer_applies_last_act=True)), else 0."""
        tower = getattr(self.bot_l, "module", self.bot_l)          # DDP / FlatDDP keep the FusedMLP in .module
        ok = _functional.FUSE_ACT_BWD and self.arch_interaction_op == "dot" and isinstance(tower, FusedMLP) and tower.ends_in_relu()
        return ops.INTERACT_RELU_X if ok else 0

    def _bags(self, lS_o, lS_i, v_W_l) -> BagBatch:
        return BagBatch(lS_o, lS_i, None)        # pooling weights, if any, are gathered on the device inside EmbeddingBagsFunction

    def _pool_weights(self, v_W_l, device) -> list:
        if v_W_l is None or not any(w is not None for w in v_W_l):
            return []
        if any(w is None for w in v_W_l):
            sys.exit("ERROR: pooling weights must be given for all tables or for none")
        out = []
        for k, w in enumerate(v_W_l):
            if w.device != device:                       # "fixed" weights are plain tensors the reference moves by hand (:1324-1326)
                w = w.to(device)
                if not isinstance(v_W_l, nn.ParameterList):
                    v_W_l[k] = w
            out.append(w)
        return out

    def _emb_weights(self, emb_l) -> List[torch.Tensor]:
        """the tables as the kernels see them: the VIRTUAL table list, where a QR table is its weight_q followed by its weight_r"""
        out = []
        for e in emb_l:
            if isinstance(e, QREmbeddingBagHolder):
                out += [e.weight_q, e.weight_r]
            elif isinstance(e, PrEmbeddingBagHolder):
                out.append(e.embs.weight)                # (its projection is a dense parameter: the optimizer's own business)
            else:
                out.append(e.weight)
        return out

    @staticmethod
    def _has_md(emb_l) -> bool:
        return emb_l is not None and any(isinstance(e, PrEmbeddingBagHolder) for e in emb_l)

    @staticmethod
    def _has_qr(emb_l) -> bool:
        return emb_l is not None and any(isinstance(e, QREmbeddingBagHolder) for e in emb_l)

    @staticmethod
    def _emb_dim(emb_l) -> int:
        e = emb_l[0]
        if isinstance(e, PrEmbeddingBagHolder):
            return e.base_dim
        return int((e.weight_q if isinstance(e, QREmbeddingBagHolder) else e.weight).size(1))

    @staticmethod
    def _md_base(emb_l) -> int:
        return next(e.base_dim for e in emb_l if isinstance(e, PrEmbeddingBagHolder))

    def _qr_spec(self, emb_l):
        """(rows, collisions, operation, keep the two pooled sums for backward) of QREmbeddingBagsFunction"""
        qr = [isinstance(e, QREmbeddingBagHolder) for e in emb_l]
        rows = [e.num_categories if q else int(e.weight.size(0)) for e, q in zip(emb_l, qr)]
        coll = [e.num_collisions if q else 0 for e, q in zip(emb_l, qr)]
        ops_ = {e.operation for e, q in zip(emb_l, qr) if q}
        if len(ops_) != 1:
            sys.exit("ERROR: all QR tables of a model must share one --qr-operation")
        return rows, coll, ops_.pop(), torch.is_grad_enabled()

    def _emb_packed(self, lS_o, lS_i, emb_l, v_W_l, out_slot: Optional[OutSlot] = None):
        """[B, T*D] pooled embeddings of all given tables, one kernel launch."""
        bags = self._bags(lS_o, lS_i, v_W_l)
        ws = self._emb_weights(emb_l)
        if self._has_qr(emb_l):
            # the QR lookup (dlrm_emb_fwd_qr) for ALL tables of the list, plain ones included; backward splits the gradient into the two
            # component gradients and hands the virtual table list to the same sink
            if v_W_l is not None and any(w is not None for w in v_W_l):
                sys.exit("ERROR: quotient remainder with weighted pooling is not supported")
            return QREmbeddingBagsFunction.apply(self._stash_embedding_grad, bags, out_slot, self._qr_spec(emb_l), *ws)
        if self._has_md(emb_l):
            # the MD lookup + projection (dlrm_emb_fwd_md) for ALL tables of the list, plain ones included (identity); backward hands each
            # width group to the same sink and returns the dense projection gradients
            if v_W_l is not None and any(w is not None for w in v_W_l):
                sys.exit("ERROR: mixed dimensions with weighted pooling is not supported")
            projs = [e.proj_weight() if isinstance(e, PrEmbeddingBagHolder) else None for e in emb_l]
            spec = (self._md_base(emb_l), [p is not None for p in projs], torch.is_grad_enabled())
            return MDEmbeddingBagsFunction.apply(self._stash_embedding_grad, bags, out_slot, spec, *ws, *[p for p in projs if p is not None])
        if self.emb_bf16 is not None and (isinstance(v_W_l, nn.ParameterList) or any(isinstance(w, nn.Parameter) for w in (v_W_l or []) if w is not None)):
            sys.exit("ERROR: bfloat16 embedding tables with learned pooling weights are not supported (the pooling-weight gradient "
                     "kernel reads fp32 rows); use --weighted-pooling=fixed")
        return EmbeddingBagsFunction.apply(self._stash_embedding_grad, bags, out_slot, *ws, *self._pool_weights(v_W_l, ws[0].device))

    def apply_emb(self, lS_o, lS_i, emb_l, v_W_l):
        """Reference-shaped result: a list with one [B, D] tensor per table (dlrm_s_pytorch.py:407-462)."""
        if self.quantize_emb:
            # (dlrm_s_pytorch.py:430-450, without its "quantized emb sizes" debug line; the tables are constants: no autograd node)
            B = len(lS_o[0])
            packed = self._emb_quant_into(lS_o, lS_i, v_W_l, torch.empty((B, len(self.emb_l_q) * self.emb_q_dim), dtype=torch.float32,
                                                                         device=self.emb_l_q[0].device))
            return list(packed.split(self.emb_q_dim, dim=1))
        packed = self._emb_packed(lS_o, lS_i, emb_l, v_W_l)
        D = self._emb_dim(emb_l)
        return list(packed.split(D, dim=1))

    def _emb_quant_into(self, lS_o, lS_i, v_W_l, out):
        """pooled rows of the packed tables (dlrm_emb_fwd_quant), all tables in one launch, written into `out` ([B, >= T*D], row stride free)"""
        bags = self._bags(lS_o, lS_i, v_W_l)
        vws = self._pool_weights(v_W_l, out.device)
        if vws:
            ops.pool_weights_gather([w.detach() for w in vws], bags)       # psw = v_W[idx], on the device (dlrm_s_pytorch.py:425-426)
        return ops.emb_fwd_quant(self.emb_l_q, self.emb_q_rows, self.emb_q_dim, self.quantize_bits, bags, out)

    def weighted_bce(self, Z, T):
        """The whole wbce loss of the reference's loss_fn_wrap (mean of loss_ws[T.long()] * BCE(Z, T), dlrm_s_pytorch.py:
        150-156) in ONE fused kernel pass — for loops that call the model directly instead of through loss_fn_wrap."""
        ws = self.loss_ws.tolist()
        return BCELossFunction.apply(Z, T, None, (ws[0], ws[1] if len(ws) > 1 else ws[0]))

    def interact_features(self, x, ly):
        if self.arch_interaction_op == "dot":
            D = x.size(1)
            return InteractFunction.apply(D, self._interaction_mode(), False, x, *ly)
        if self.arch_interaction_op == "cat":
            return CatFunction.apply(None, x, *ly)
        sys.exit("ERROR: --arch-interaction-op=" + str(self.arch_interaction_op) + " is not supported")

    def quantize_embedding(self, bits):
        """dlrm_s_pytorch.py:465-481 on the device: emb_l_q[k] = table k in torch's fused row-wise format (uint8 [rows, D + 8] at 8 bits,
        [rows, D/2 + 4] at 4 bits: byte for byte `ops.quantized.embedding_bag_{byte,4bit}_prepack` of the same weights), emb_l = None.
        Any other `bits` returns without change, as in the reference.  Tables are packed and released one by one (peak: the fp32 tables
        plus one packed table).  From here on the model is an inference model: its lookups go through dlrm_emb_fwd_quant."""
        if bits not in (4, 8):
            return
        if self.emb_bf16 is not None:
            sys.exit("ERROR: 4 and 8-bit quantization with bfloat16 embedding tables is not supported (quantize the fp32 model)")
        if self._has_qr(self.emb_l):
            sys.exit("ERROR: 4 and 8-bit quantization with quotient remainder is not supported")
        if self._has_md(self.emb_l):
            sys.exit("ERROR: 4 and 8-bit quantization with mixed dimensions is not supported")
        if self.quantize_emb:
            sys.exit("ERROR: the embedding tables are quantized already (%d bits)" % self.quantize_bits)
        if ext_dist.is_distributed():
            sys.exit("ERROR: quantized embedding tables are single-process inference only (distributed quantized inference is not built)")
        if self.update_in_backward:
            sys.exit("ERROR: update_in_backward trains the embedding tables; quantized tables are constants (inference only)")
        if self._pending_emb:
            sys.exit("ERROR: an embedding update is still parked (backward without optimizer.step()); step or drop it before quantize_embedding")
        weights = self._emb_weights(self.emb_l)
        if not weights or any(not w.is_cuda for w in weights):
            raise RuntimeError("dlrm_amd: quantize_embedding packs the tables on the GPU and the quantized lookup has no CPU path; "
                               "move the model to the device first (model.to('cuda'))")
        self._join_side_stream()
        n = len(self.emb_l)
        self.emb_q_rows = [int(w.size(0)) for w in weights]
        self.emb_q_dim = int(weights[0].size(1))
        ops.quant_row_bytes(self.emb_q_dim, bits)                       # (4 bits need an even dimension: refused before anything changes)
        self._emb_fp32_refs = [weakref.ref(w) for w in weights]         # an optimizer that still holds one of them must not step: _refuse_step
        del weights
        self.emb_l_q = [None] * n
        for k in range(n):
            self.emb_l_q[k] = ops.emb_quantize(self.emb_l[k].weight.detach(), bits)
            self.emb_l[k].weight = None                                  # release the fp32 rows of this table before the next one is packed
        self.emb_l = None
        self.quantize_emb = True
        self.quantize_bits = bits

    def _refuse_bf16(self, learned_pooling: bool, has_qr: bool, has_md: bool) -> None:
        """every configuration bfloat16 tables are not built for, refused before anything is modified"""
        if not self._bf16_supported:
            sys.exit("ERROR: bfloat16 embedding tables are built for DLRM_Net only, not for the torchrec variants (%s)" % type(self).__name__)
        if has_qr:
            sys.exit("ERROR: bfloat16 embedding tables with quotient remainder are not supported")
        if has_md:
            sys.exit("ERROR: bfloat16 embedding tables with mixed dimensions are not supported")
        if learned_pooling:
            sys.exit("ERROR: bfloat16 embedding tables with learned pooling weights are not supported (the pooling-weight gradient "
                     "kernel reads fp32 rows); use --weighted-pooling=fixed")
        if not self.fused_emb_update:
            sys.exit(UPDATE_REFUSALS["unfused", "bf16"])
        if ext_dist.is_distributed():
            sys.exit("ERROR: bfloat16 embedding tables are single-process only (the table-sharded distributed forward is not built for them)")

    def embedding_bfloat16(self, rounding: str = "stochastic", seed: int = 0) -> None:
        """Store every embedding table in bfloat16 (half the table bytes, half the row traffic of the HBM-bound lookup and update kernels).
        Tables are converted in place, one by one, round-to-nearest (`p.data = p.data.to(torch.bfloat16)`: the Parameter objects stay, an
        optimizer built earlier still owns them; peak memory = the fp32 tables plus one bf16 table); state_dict keys are unchanged, its
        table entries are bfloat16, and loading an fp32 checkpoint casts.
        Forward: dlrm_emb_fwd_bf16 + the interaction kernel — the bits of the fp32 model on the upcast tables (the fp32 fused lookup +
        interaction kernels are not entered; with fuse_bf16_interact = True the bf16 ones of csrc/interact_bf16.hip are, forward and
        backward, for the same bits; update_in_backward falls back to the step-time update).
        Update (plain SGD or row-wise Adagrad, when the optimizer steps): the gradient of a row is summed in fp32, the row is stepped in
        fp32 and rounded ONCE per update call — rounding = "stochastic" (default; Philox keyed by (seed, number of update calls so far), so a
        run is reproducible) or "nearest".  Gradient accumulation with SGD applies each parked backward pass in turn: one rounding per
        pass, not one per optimizer step."""
        if rounding not in ops.BF16_ROUNDINGS:
            sys.exit("ERROR: bfloat16 embedding tables round 'stochastic' or 'nearest', got " + repr(rounding))
        if self.emb_bf16 is not None:
            sys.exit("ERROR: the embedding tables are bfloat16 already")
        if getattr(self, "quantize_emb", False):
            sys.exit("ERROR: the embedding tables are quantized (%d bits); bfloat16 tables are built from the fp32 model" % self.quantize_bits)
        self._refuse_bf16(isinstance(self.v_W_l, nn.ParameterList), self._has_qr(self.emb_l), self._has_md(self.emb_l))
        if self._pending_emb:
            sys.exit("ERROR: an embedding update is still parked (backward without optimizer.step()); step or drop it before embedding_bfloat16")
        self._join_side_stream()
        for e in self.emb_l:
            e.weight.data = e.weight.data.to(torch.bfloat16)             # one table at a time: its fp32 rows are released here
        self.emb_bf16 = (rounding, int(seed))
        self._bf16_update_calls = 0

    def _bf16_next_seed(self) -> int:
        n = self._bf16_update_calls
        self._bf16_update_calls = n + 1
        return _mix_seed(self.emb_bf16[1], n)

    def _run_update(self, plan, weights, bags, dout) -> None:
        """The ONE place that maps an update plan — ("sgd", lr), ("rwsadagrad", clr, eps, states) or ("adagrad", clr, eps, sums), as
        _embedding_update_plan builds them — to the fused backward + update kernel of one backward pass: the fp32 kernels, or the bf16 ones
        (this model's rounding, one seed of its counter per call) for bfloat16 tables.  What no kernel is built for was refused before
        (UPDATE_REFUSALS)."""
        kind = plan[0]
        if self.emb_bf16 is not None:
            dev_state = ops.device_step_state(self)
            if dev_state is not None:
                # a whole-step graph is capturing (graph.py, device_step_state): the key is drawn ON THE DEVICE, from the counter the replays advance
                ops.philox_key_next(self.emb_bf16[1], dev_state.calls, dev_state.key)
                dev_state.draws += 1
                seed = dev_state.key
            else:
                if self._step_state_settle is not None:
                    self._step_state_settle()                 # (replays of such a graph advanced the device counter: the host one follows first)
                seed = self._bf16_next_seed()
            if kind == "sgd":
                ops.emb_bwd_sgd_bf16(weights, bags, dout, plan[1], self.emb_bf16[0], seed)
            else:
                ops.emb_bwd_rowwise_adagrad_bf16(weights, plan[3], bags, dout, plan[1], plan[2], self.emb_bf16[0], seed)
        elif kind == "sgd":
            ops.emb_bwd_sgd(weights, bags, dout, plan[1], self.emb_update_mode)
        elif kind == "rwsadagrad":
            ops.emb_bwd_rowwise_adagrad(weights, plan[3], bags, dout, plan[1], plan[2])
        else:
            ops.emb_bwd_adagrad(weights, plan[3], bags, dout, plan[1], plan[2])

    def _refuse_update(self, update: str) -> None:
        """exit with the message of UPDATE_REFUSALS if `update` is not built for this model's tables"""
        msg = UPDATE_REFUSALS.get((update, self._table_kind()))
        if msg is not None:
            sys.exit(msg)

    def quantize_mlp(self, bits):
        """The reference's `torch.quantization.quantize_dynamic(dlrm, {torch.nn.Linear}, qint8 | float16)` of --quantize-mlp-with-bit 8 | 16
        (dlrm_s_pytorch.py:1473-1480) on the device: both towers become inference towers (FusedMLP.quantize).  Any other `bits` returns
        without change, as the reference does for 32.  Every refusal comes before anything is modified."""
        if bits not in (8, 16):
            return
        if self.quantize_mlp_bits != 32:
            sys.exit("ERROR: the MLP towers are quantized already (%d bits)" % self.quantize_mlp_bits)
        if self._has_md(self.emb_l):
            sys.exit("ERROR: quantized MLP towers with mixed dimensions are not supported (quantize_dynamic would also quantize the "
                     "tables' projections, which is not built)")
        if ext_dist.is_distributed():
            sys.exit("ERROR: quantized MLP towers are single-process inference only (distributed quantized inference is not built)")
        towers = (self.bot_l, self.top_l)
        if any(not isinstance(t, FusedMLP) for t in towers):
            sys.exit("ERROR: quantized MLP towers are single-process inference only (a DistributedDataParallel-wrapped tower cannot be "
                     "quantized)")
        if any(t.quant_bits != 32 for t in towers):
            sys.exit("ERROR: the MLP towers are quantized already")
        if any(not p.is_cuda for t in towers for p in t.parameters()):
            raise RuntimeError("dlrm_amd: quantize_mlp packs the towers on the GPU and the quantized layers have no CPU path; "
                               "move the model to the device first (model.to('cuda'))")
        for t in towers:
            t._layers()                                               # (a tower that is not Linear + activation raises here)
        self._join_side_stream()
        for t in towers:
            t.quantize(bits)
        self.quantize_mlp_bits = bits

    # (the towers refuse these themselves; asked here first, so that no table has been moved or loaded before the refusal)
    def _apply(self, fn, *args, **kwargs):
        if self.quantize_mlp_bits != 32:
            sys.exit("ERROR: a model with quantized MLP towers (%d bits) cannot be moved or converted (.to / .cuda / .cpu / .half): the "
                     "towers' packed weights live on the device they were packed on" % self.quantize_mlp_bits)
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        if self.quantize_mlp_bits != 32:
            sys.exit("ERROR: load_state_dict into a model with quantized MLP towers (%d bits): quantized towers are constants (inference "
                     "only) — load the fp32 weights first, then quantize_mlp" % self.quantize_mlp_bits)
        return super().load_state_dict(*args, **kwargs)

    def _refuse_step_if_mlp_quantized(self, optimizer) -> None:
        mine = {id(p) for t in (self.bot_l, self.top_l) for p in t.parameters()}
        if any(id(p) in mine for g in optimizer.param_groups for p in g["params"]):
            sys.exit("ERROR: this optimizer holds the parameters of MLP towers that are quantized now (%d bits); quantized towers are "
                     "constants (inference only)" % self.quantize_mlp_bits)

    def _refuse_step_if_quantized(self, optimizer) -> None:
        if not self.quantize_emb:
            return
        old = {id(w) for w in (r() for r in getattr(self, "_emb_fp32_refs", [])) if w is not None}
        if old and any(id(p) in old for g in optimizer.param_groups for p in g["params"]):
            sys.exit("ERROR: this optimizer holds the fp32 embedding tables of a model whose tables are quantized now; quantized tables "
                     "are constants (inference only) — build the optimizer over model.parameters() after quantize_embedding")

    # ---------------------------------------------------------------- fused sparse update
    def _owned_by(self, optimizer) -> bool:
        mine = {id(w) for w in self._emb_weights(self.emb_l)}
        return any(id(p) in mine for g in optimizer.param_groups for p in g["params"])

    def _join_side_stream(self) -> None:
        if self._side_keep:
            dev = self._side_keep[0].device
            ops.timer_mark()
            torch.cuda.current_stream(dev).wait_stream(_side_stream(dev))
            self._side_keep = []

    def _presort_for_backward(self, weights, bags, pred):
        """`bags.presort` of the fused lookup + interaction path (GatherInteractFunction.backward): ops.Presorted when this backward pass may
        take the SGD step of single-lookup rows itself (update_in_backward, a bound plain-SGD optimizer, the sorted update, nothing parked,
        not inside a distributed forward), else None."""
        if not (self.update_in_backward and self.fused_emb_update and self.emb_update_mode == ops.UPD_SORTED) or self._pending_emb:
            return None
        opt = self._bound_optimizer() if self._bound_optimizer is not None else None
        if opt is None or not _is_plain_sgd(opt) or not ops.presort_ok(weights, bags):
            return None
        plan = _embedding_update_plan(opt, weights)
        if plan is None or plan[0] != "sgd":
            return None
        return ops.emb_presort(weights, bags, plan[1], pred)

    @contextlib.contextmanager
    def _on_side_stream(self, device, keep, always_wait=False):
        """What is launched inside runs on the device's side stream, after everything the current stream holds now; `keep`, the tensors those
        launches read, stay alive until the join (_join_side_stream).  A backward node whose forward ran on the side stream is on it already
        and waits for nothing (always_wait: the caller is never on it)."""
        cur, side = torch.cuda.current_stream(device), _side_stream(device)
        if always_wait or cur != side:           # (cur != side in a backward node: distributed forward, the lookups ran on the main stream)
            ops.timer_mark()
            side.wait_stream(cur)
        self._side_keep += keep
        with torch.cuda.stream(side):
            yield

    def _stash_embedding_grad(self, weights, bags, dout, presorted=None):
        # (overlap mode: the optimizer that owns the tables, once known from its earlier steps)
        bound = self._bound_optimizer() if (self.overlap_streams and self._bound_optimizer is not None) else None
        if presorted is not None:
            # the fused backward already applied the single-lookup rows with presorted.lr; the rest follows from the same sorted workspace —
            # on the side stream now (overlap mode) or when the optimizer steps
            if bound is not None:
                with self._on_side_stream(dout.device, [dout, presorted.ws, presorted.mask] + bags.keep):
                    ops.emb_bwd_sgd_presorted(weights, bags, dout, presorted)
            else:
                self._pending_emb.append(ParkedGrad(weights, bags, dout, presorted))
            return
        if not self.fused_emb_update:
            self._refuse_update("unfused")
            self._materialize_coo_grads(weights, bags, dout)
            return
        if bound is not None and not self._pending_emb:
            # the sparse SGD update is launched NOW — this backward node runs on the side stream its forward ran on, so the update
            # overlaps the bottom-MLP backward that autograd runs next on the main stream — with the learning rate the optimizer
            # holds at this moment (the reference reads it at step(), a few microseconds later in the same loop body:
            # dlrm_s_pytorch.py:1611-1621)
            plan = _embedding_update_plan(bound, weights) if _is_plain_sgd(bound) else None     # (the Adagrad plan advances state["step"]: only built where it is applied)
            if plan is not None and plan[0] == "sgd":
                with self._on_side_stream(dout.device, [dout] + bags.keep):
                    self._run_update(plan, weights, bags, dout)
                return
        self._pending_emb.append(ParkedGrad(weights, bags, dout))
        if len(self._pending_emb) == 65:
            print("WARNING: dlrm_amd: 65 embedding gradients are parked and no optimizer that owns the tables has stepped; "
                  "every backward() keeps its [B, T*D] gradient buffer alive until then", file=sys.stderr)

    @staticmethod
    def _materialize_coo_grads(weights, bags, dout):
        """emb.weight.grad (+)= the reference's sparse COO gradient: indices = the lookup indices verbatim (uncoalesced),
        values = dout[bag(i)] * psw[i] (EmbeddingBagBackward, dlrm_s_pytorch.py:1613)."""
        if getattr(bags, "ignore_oob", False):
            sys.exit("ERROR: fused_emb_update = False (sparse COO gradients) cannot be combined with row-wise table shards, whose "
                     "out-of-range ids are other ranks' rows")
        ops.check_index_errors(sync=True)        # the reference raises in forward; never hand an out-of-range id to an optimizer's scatter
        D = weights[0].size(1)
        values = ops.emb_bwd_coo(bags, dout, D)
        for k, (w, v) in enumerate(zip(weights, values)):
            idx = ops.bag_index_tensor(bags, k).reshape(1, -1).long()
            g = torch.sparse_coo_tensor(idx, v, size=tuple(w.shape), check_invariants=False)
            w.grad = g if w.grad is None else w.grad + g

    def apply_pending_embedding_updates(self, optimizer=None, lr: Optional[float] = None) -> None:
        """Launch the fused backward+update for every stashed embedding gradient: sparse SGD for torch.optim.SGD,
        row-wise sparse Adagrad for RWSAdagrad (the reference's optim/rwsadagrad.py or dlrm_amd.optim.FusedRWSAdagrad)."""
        pending, self._pending_emb = self._pending_emb, []
        if self.overlap_streams and pending and pending[0].dout.is_cuda:
            # launched from the step pre-hook: on the side stream, beside the dense optimizer step (joined in the post-hook)
            keep = [p_.dout for p_ in pending] + [t for p_ in pending for t in p_.bags.keep]
            keep += [t for p_ in pending if p_.presorted is not None for t in (p_.presorted.ws, p_.presorted.mask)]
            with self._on_side_stream(pending[0].dout.device, keep, always_wait=True):
                if optimizer is not None and self._bound_optimizer is None and self._owned_by(optimizer):
                    self._bound_optimizer = weakref.ref(optimizer)
                self._apply_pending(pending, optimizer, lr)
        else:
            self._apply_pending(pending, optimizer, lr)

    def _apply_pending(self, pending, optimizer, lr):
        pending = [ParkedGrad(*entry) for entry in pending]
        dev_state = ops.device_step_state(self)
        if dev_state is not None:
            dev_state.passes += len(pending)                      # (what a capturing whole-step graph checks its key draws against)
        for weights, bags, dout, pre in pending:
            if pre is not None:
                # (the backward pass already took the single-lookup rows with pre.lr — the optimizer's lr then; the rest takes the same step size)
                ops.emb_bwd_sgd_presorted(weights, bags, dout, pre)
                continue
            if lr is not None:
                self._run_update(("sgd", lr), weights, bags, dout)
                continue
            # parked backward passes over THESE tables (`weights` is a fresh tuple per forward call: compare the tables themselves)
            key = tuple(id(w) for w in weights)
            if _is_exact_adagrad(optimizer, self.fused_adagrad) and self._owned_by(optimizer):
                self._refuse_update("adagrad")                    # (asked in front of the plan, which advances state["step"])
            plan = _embedding_update_plan(optimizer, weights, count=sum(1 for p_ in pending if tuple(id(w) for w in p_.weights) == key),
                                          fused_adagrad=self.fused_adagrad)
            if plan is None:
                self._pending_emb.append(ParkedGrad(weights, bags, dout))   # another optimizer owns these tables
                continue
            if plan[0] != "sgd":                                  # (nothing refuses plain SGD: the per-step path does not ask)
                self._refuse_update(plan[0])
            if plan[0] == "coo":
                self._materialize_coo_grads(weights, bags, dout)  # the optimizer's own step consumes .grad right after this hook
            else:
                self._run_update(plan, weights, bags, dout)

    # ---------------------------------------------------------------- forward paths
    def forward(self, dense_x, lS_o, lS_i):
        if ext_dist.is_distributed():        # more than one rank (or a forced one-rank RCCL group: ext_dist.force_distributed)
            return self.distributed_forward(dense_x, lS_o, lS_i)
        return self.sequential_forward(dense_x, lS_o, lS_i)

    def _clamp(self, p):
        if 0.0 < self.loss_threshold < 1.0:
            return ClampFunction.apply(p, float(self.loss_threshold), float(1.0 - self.loss_threshold))
        return p

    def sequential_forward(self, dense_x, lS_o, lS_i):
        """bottom MLP -> embeddings -> interaction -> top MLP (dlrm_s_pytorch.py:587-612): the fused lookup + interaction form where a route
        and the batch admit it (_fused_forward), else the two-kernel form, with the bottom tower and the embedding kernel writing directly
        into the [B, (1+T)*D] feature buffer."""
        if self.arch_interaction_op not in ("dot", "cat"):
            sys.exit("ERROR: --arch-interaction-op=" + str(self.arch_interaction_op) + " is not supported")
        ops.check_index_errors()          # host memory read, no synchronisation: bad indices of earlier steps surface here
        B = dense_x.size(0)
        quant = self.quantize_emb
        if quant:
            T, D = len(self.emb_l_q), self.emb_q_dim
            if self.update_in_backward:
                sys.exit("ERROR: update_in_backward trains the embedding tables; quantized tables are constants (inference only)")
        else:
            T = len(self.emb_l)
            D = self._emb_dim(self.emb_l)
        n_out = self.bot_l[-2].out_features if isinstance(self.bot_l[-2], nn.Linear) else D
        if self.arch_interaction_op == "dot" and n_out != D:
            sys.exit("ERROR: bottom MLP output (%d) and embedding dimension (%d) differ" % (n_out, D))
        # the last ReLU of the bottom tower is differentiated inside the interaction backward (which has x staged): see _relu_x
        rx = self._relu_x() if dense_x.is_cuda else 0
        z = self._fused_forward(dense_x, lS_o, lS_i, B, T, D, rx)
        if z is not None:
            return self._clamp(self.apply_mlp(z, self.top_l))
        # the two-kernel form: the bottom tower writes its slot of the feature buffer, the lookup (dlrm_emb_fwd_quant for packed tables) the rest
        feat = torch.empty((B, n_out + T * D), dtype=torch.float32, device=dense_x.device)
        if self.overlap_streams and dense_x.is_cuda and not quant:
            # pooled lookups (HBM-bound) on the side stream beside the bottom-MLP GEMMs (MFMA-bound): they only meet at the
            # interaction.  The side stream first waits for everything already enqueued (inputs, the previous update).
            main, side = torch.cuda.current_stream(dense_x.device), _side_stream(dense_x.device)
            ops.timer_mark()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                E = self._emb_packed(lS_o, lS_i, self.emb_l, self.v_W_l, out_slot=OutSlot(feat[:, n_out:]))
            x = self.apply_mlp(dense_x, self.bot_l, out_slot=OutSlot(feat[:, :n_out]), consumer_applies_last_act=bool(rx))
            ops.timer_mark()
            main.wait_stream(side)
        else:
            x = self.apply_mlp(dense_x, self.bot_l, out_slot=OutSlot(feat[:, :n_out]), consumer_applies_last_act=bool(rx))
            if quant:
                E = self._emb_quant_into(lS_o, lS_i, self.v_W_l, feat[:, n_out:])
            else:
                E = self._emb_packed(lS_o, lS_i, self.emb_l, self.v_W_l, out_slot=OutSlot(feat[:, n_out:]))
        if self.arch_interaction_op == "cat":
            z = CatFunction.apply(OutSlot(feat), x, E)      # the feature buffer IS cat([x] + ly, 1): nothing is copied
        else:
            z = InteractFunction.apply(D, self._interaction_mode() | rx, True, x, E)   # [B, round4(width)], zero padded
        return self._clamp(self.apply_mlp(z, self.top_l))

    def _table_kind(self) -> str:
        """the `tables` argument of fused_route (a QR list stored as bfloat16 — refused at construction — stays "qr": see its bf16_rows)"""
        if self.quantize_emb:
            return "quant"
        kind = "fp32" if self.emb_bf16 is None else "bf16"
        for e in self.emb_l:
            if isinstance(e, (PrEmbeddingBagHolder, QREmbeddingBagHolder)):       # (one test per plain table: this runs at every step)
                if isinstance(e, PrEmbeddingBagHolder):
                    return "md"
                kind = "qr"
        return kind

    def fused_route_now(self, tables: Optional[str] = None, T: Optional[int] = None, D: Optional[int] = None,
                        grad_wanted: bool = False) -> Optional[FusedRoute]:
        """fused_route for this model as it is now, on a GPU batch: THE place that reads the model's attributes for it (_fused_forward at
        every step, which passes the table kind and sizes it already has; GraphedForward and GraphedTrainStep to learn whether an offsets
        proof is worth its host wait).  None: the two-kernel form."""
        tables = self._table_kind() if tables is None else tables
        packed = tables == "quant"
        if T is None:
            T, D = (len(self.emb_l_q), self.emb_q_dim) if packed else (len(self.emb_l), self._emb_dim(self.emb_l))
        return fused_route(
            tables, 1 + T, D, self.quantize_bits if packed else 0, fuse_emb_interact=self.fuse_emb_interact,
            fuse_quant_interact=self.fuse_quant_interact, fuse_qr_interact=self.fuse_qr_interact, fuse_bf16_interact=self.fuse_bf16_interact,
            fuse_narrow_interact=self.fuse_narrow_interact, update_in_backward=self.update_in_backward,
            interaction_op=self.arch_interaction_op, pooling_weights=any(w is not None for w in (self.v_W_l or [])),
            grad_wanted=grad_wanted, bf16_rows=self.emb_bf16 is not None)

    def _fused_forward(self, dense_x, lS_o, lS_i, B, T, D, rx):
        """The interaction output through the fused lookup + interaction kernels of the route fused_route picks, or None: the two-kernel form.
        What the route cannot know is asked here: B lookups per table, every table's base address a multiple of route.align bytes (one lane's
        load: ops.RowKind.align), and the offsets' state (_fused_bottom).  Undecided offsets (a HIP graph is being captured) run the fused
        kernels alone where route.none_fused says so: GraphedTrainStep proves every incoming batch, for the shapes of ops.gather_ok.
        Packed tables (route.autograd False) are constants: no autograd node, the bottom tower keeps its own last activation, and a forward
        whose bottom tower is being trained is no route at all (InteractFunction carries the gradient of x)."""
        if not (self.fuse_emb_interact and self.arch_interaction_op == "dot" and dense_x.is_cuda):
            return None                     # (fused_route's first three conditions, asked before anything is looked at)
        tables = self._table_kind()
        packed = tables == "quant"
        route = self.fused_route_now(tables, T, D, grad_wanted=packed and torch.is_grad_enabled() and (dense_x.requires_grad or (
            getattr(self.bot_l, "quant_bits", 32) == 32 and any(p_.requires_grad for p_ in self.bot_l.parameters()))))
        if route is None:
            return None
        bags = self._bags(lS_o, lS_i, None)
        ws = self.emb_l_q if packed else self._emb_weights(self.emb_l)
        if not (all(n == B for n in bags.nnz) and ops.tables_aligned(ws, route.align)):
            return None
        if not route.autograd:
            rx = 0
        x = self._fused_bottom(dense_x, lS_o, bags, rx, route.none_fused, route.host_proof)
        if x is None:
            return None
        if not route.autograd:
            return _functional.gather_interact_fwd(None, None, route.kind, (self.emb_q_rows, D, self.quantize_bits), D,
                                                   self._interaction_mode(), bags, x, ws)
        # (the update inside the backward exists for fp32 tables of D = 128 only: everywhere else update_in_backward falls back to the step-time update)
        bags.presort = self._presort_for_backward if route.presort else None
        spec = self._qr_spec(self.emb_l) if tables == "qr" else None
        return GatherInteractFunction.apply(self._stash_embedding_grad, route.kind, spec, D, self._interaction_mode() | rx, bags, x, *ws)

    def _fused_bottom(self, dense_x, lS_o, bags, rx, none_fused, host_proof=True):
        """The offsets decision of the fused paths, with the bottom tower in its middle -> the tower's output x with bags.iota_flag set, or None:
        the two-kernel form (where the verdict came only after the tower, the tower runs again, into its slot).
        nnz == B does not prove one lookup per bag (an empty bag next to a two-lookup bag is legal EmbeddingBag input and the reference
        computes it): dlrm_amd/iota.py proves offsets == arange(B) on the device, once per offsets tensor object.  True -> the fused kernels
        alone (iota_flag None).  A tensor nobody vouched for -> its proof is a device pass whose verdict STAYS on the device: iota_flag is that
        flag, the Function enqueues the fused kernels and the two-kernel form, each behind the launch predicate, and the host goes on.  False
        (this tensor object was proven ragged before) -> None.  None (undecided, only while a HIP graph is being captured) -> the fused
        kernels alone if `none_fused`, else None.
        DLRM_DEVICE_PREDICATE=0 with `host_proof`: the host-side proof — started on its own stream, the bottom tower enqueued, then the host
        waits for the verdict — kept for A/B and for the tests of that path."""
        proof = None
        if DEVICE_PREDICATE or not host_proof:
            state = ops.offsets_iota_state(lS_o)
        else:
            proof = ops.offsets_are_iota_start(lS_o)
            state = proof if (proof is None or isinstance(proof, bool)) else "pending"
        if state is False or (state is None and not none_fused):
            return None
        x = self.apply_mlp(dense_x, self.bot_l, consumer_applies_last_act=bool(rx))
        if proof is not None and state == "pending":
            state = ops.offsets_are_iota_finish(proof)
            if state is False or (state is None and not none_fused):
                return None
        bags.iota_flag = state if isinstance(state, torch.Tensor) else None
        return x

    def distributed_forward(self, dense_x, lS_o, lS_i):
        """Table-wise sharded embeddings + batch-split MLPs (dlrm_s_pytorch.py:528-585): every rank pools
        the WHOLE batch for its tables, one all-to-all turns table-split into batch-split, the bottom
        MLP runs while the exchange is in flight."""
        if self.quantize_emb:
            sys.exit("ERROR: quantized embedding tables are single-process inference only (distributed quantized inference is not built)")
        if self.emb_bf16 is not None:
            sys.exit("ERROR: bfloat16 embedding tables are single-process only (the table-sharded distributed forward is not built for them)")
        if self._has_qr(self.emb_l):
            sys.exit("ERROR: QR embedding tables are single-process only (the table-sharded distributed forward is not built for them)")
        if self._has_md(self.emb_l):
            sys.exit("ERROR: mixed-dimension embedding tables are single-process only (the table-sharded distributed forward is not built "
                     "for them)")
        batch_size = dense_x.size(0)
        if batch_size < ext_dist.my_size:
            sys.exit("ERROR: batch_size (%d) must be larger than number of ranks (%d)" % (batch_size, ext_dist.my_size))
        if batch_size % ext_dist.my_size != 0:
            sys.exit("ERROR: batch_size %d can not split across %d ranks evenly" % (batch_size, ext_dist.my_size))
        ops.check_index_errors()
        dense_x = dense_x[ext_dist.get_my_slice(batch_size)]
        lS_o = lS_o[self.local_emb_slice]
        lS_i = lS_i[self.local_emb_slice]
        if len(self.emb_l) != len(lS_o) or len(self.emb_l) != len(lS_i):
            sys.exit("ERROR: corrupted model input detected in distributed_forward call")
        D = self.emb_l[0].weight.size(1)
        E = self._emb_packed(lS_o, lS_i, self.emb_l, self.v_W_l)           # [B, T_loc*D] == packed send buffer
        C = self.a2a_chunks
        if C > 1 and self.arch_interaction_op == "dot" and (batch_size // ext_dist.my_size) % C == 0:
            return self._pipelined_exchange_forward(dense_x, E, D, batch_size, C)
        req = ext_dist.alltoall([E], self.n_emb_per_rank, emb_dim=D)
        rx = self._relu_x() if dense_x.is_cuda else 0                       # (see sequential_forward)
        x = self.apply_mlp(dense_x, self.bot_l, consumer_applies_last_act=bool(rx))     # overlaps the exchange
        ly = list(req.wait())                                               # N x [B/N, T_s*D], read in place
        if self.arch_interaction_op == "dot":
            z = InteractFunction.apply(D, self._interaction_mode() | rx, True, x, *ly)
        else:
            z = self.interact_features(x, ly)
        return self._clamp(self.apply_mlp(z, self.top_l))

    def _pipelined_exchange_forward(self, dense_x, E, D, batch_size, C):
        """Distributed forward with the all-to-all split into C batch chunks (opt-in, DLRM_A2A_CHUNKS / model.a2a_chunks).

        The exchange moves B*T_loc*D*4*(N-1)/N bytes per rank and direction over N-1 xGMI links (218 MB over ONE link at
        N = 2) while only the bottom MLP overlaps it in the reference schedule (dlrm_s_pytorch.py:563-568).  Here all C chunk
        exchanges are issued up front (they queue on RCCL's stream); interaction + top MLP of chunk c run while chunks
        c+1.. are still on the wire, and in backward the reverse exchange of chunk c overlaps the top-MLP backward of the
        chunks before it (the autograd engine reaches them in reverse order).  Weight gradients of the C top-MLP passes are
        summed by autograd; results equal the unchunked schedule up to fp32 summation order of those C partial gradients."""
        N = ext_dist.my_size
        Bc = batch_size // N // C
        sends = ChunkPackFunction.apply(E, N, C)
        reqs = [ext_dist.alltoall([sends[c]], self.n_emb_per_rank, emb_dim=D) for c in range(C)]
        rx = self._relu_x() if dense_x.is_cuda else 0                           # every chunk's backward masks its own rows of dx
        x = self.apply_mlp(dense_x, self.bot_l, consumer_applies_last_act=bool(rx))     # overlaps the first exchange
        outs = []
        for c in range(C):
            ly = list(reqs[c].wait())                                           # N x [Bc, T_s*D]
            z = InteractFunction.apply(D, self._interaction_mode() | rx, True, x[c * Bc:(c + 1) * Bc], *ly)
            outs.append(self.apply_mlp(z, self.top_l))
        return self._clamp(torch.cat(outs, dim=0))


def _is_plain_sgd(optimizer) -> bool:
    return isinstance(optimizer, torch.optim.SGD) and not _is_rwsadagrad(optimizer)


def _is_rwsadagrad(optimizer) -> bool:
    """The reference's RWSAdagrad (optim/rwsadagrad.py) or our FusedRWSAdagrad: recognised by name + hyper-parameters so
    that the reference class needs no import here."""
    d = getattr(optimizer, "defaults", {})
    return type(optimizer).__name__ in ("RWSAdagrad", "FusedRWSAdagrad") and \
        all(k in d for k in ("lr", "lr_decay", "eps", "initial_accumulator_value"))


def _is_exact_adagrad(optimizer, fused_adagrad=False) -> bool:
    """dlrm_amd.optim.FusedAdagrad, or — only with DLRM_Net.fused_adagrad — a stock torch.optim.Adagrad (the reference's --optimizer=adagrad)."""
    d = getattr(optimizer, "defaults", {})
    if not all(k in d for k in ("lr", "lr_decay", "eps", "initial_accumulator_value")):
        return False
    if type(optimizer).__name__ == "FusedAdagrad":
        return True
    return bool(fused_adagrad) and type(optimizer) is torch.optim.Adagrad and \
        not any(g.get("maximize", False) for g in optimizer.param_groups)


def _embedding_update_plan(optimizer, weights, count=1, fused_adagrad=False):
    """None if `optimizer` does not own the tables; ("sgd", lr) for torch.optim.SGD; ("rwsadagrad", clr, eps, states)
    for RWSAdagrad — `states` are the per-table row-wise accumulators kept in optimizer.state[p]["momentum"] exactly
    where the reference keeps them (created lazily with initial_accumulator_value, rwsadagrad.py:89-95), the step count
    in state[p]["step"] (clr = lr / (1 + (step-1)*lr_decay), :113-115); ("adagrad", clr, eps, sums) for FusedAdagrad and,
    with `fused_adagrad` (DLRM_Net.fused_adagrad), for a stock torch.optim.Adagrad — `sums` are the optimizer's own
    state[p]["sum"] tensors ([rows, D]), clr and the step count as for RWSAdagrad; ("coo",) for every other optimizer (and SGD with
    momentum / weight decay): the sparse COO gradient is materialised and the optimizer's own step consumes it, as in
    the reference.  `count` = parked backward passes of these tables (gradient accumulation)."""
    if optimizer is None:
        return None
    owner = {}
    for group in optimizer.param_groups:
        for p in group["params"]:
            owner[id(p)] = group
    groups = [owner.get(id(w)) for w in weights]
    if all(g is None for g in groups):
        return None
    if any(g is None for g in groups):
        sys.exit("ERROR: optimizer holds only some of the embedding tables")
    exact = _is_exact_adagrad(optimizer, fused_adagrad)
    if exact or _is_rwsadagrad(optimizer):
        if count > 1:
            # the reference coalesces the ACCUMULATED gradient and applies one non-linear update / one step increment;
            # several separate fused updates would not equal that
            sys.exit("ERROR: gradient accumulation (more than one backward per optimizer step) with the fused %s "
                     "Adagrad update is not supported; set model.fused_emb_update = False (DLRM_FUSED_EMB_UPDATE=0)" %
                     ("exact" if exact else "row-wise"))
        if any(g.get("weight_decay", 0) != 0 for g in groups):
            sys.exit("ERROR: weight_decay option is not compatible with sparse gradients")
        # the accumulator: torch's state["sum"], the shape of the table (exact) | the reference's state["momentum"], [rows] (row-wise)
        name = "sum" if exact else "momentum"
        clrs, states = [], []
        for w, g in zip(weights, groups):
            st = optimizer.state[w]
            if name not in st or (not exact and st[name].device != w.device):
                st[name] = torch.full(list(w.shape) if exact else [w.shape[0]], float(optimizer.defaults["initial_accumulator_value"]),
                                      dtype=torch.float32, device=w.device)
            st["step"] = st.get("step", 0) + 1          # (a python number, or torch.optim.Adagrad's host tensor)
            clrs.append(float(g["lr"]) / (1.0 + (float(st["step"]) - 1.0) * float(g["lr_decay"])))
            states.append(st[name])
        if len(set(clrs)) != 1 or len({float(g["eps"]) for g in groups}) != 1:
            sys.exit("ERROR: embedding tables in param groups with different learning rates are not supported")
        clr = clrs[0]
        if float(groups[0]["lr_decay"]) == 0.0:
            clr = ops.device_lr(groups[0], clr)          # clr == lr: the group's device scalar while a whole-step graph captures (graph.py)
        return ("adagrad" if exact else "rwsadagrad", clr, float(groups[0]["eps"]), states)
    if not isinstance(optimizer, torch.optim.SGD):
        return ("coo",)
    for g in groups:
        if g.get("momentum", 0) != 0 or g.get("weight_decay", 0) != 0 or g.get("nesterov", False) or g.get("maximize", False):
            return ("coo",)
    lrs = [float(g["lr"]) for g in groups]
    if len(set(lrs)) != 1:
        sys.exit("ERROR: embedding tables in param groups with different learning rates are not supported")
    return ("sgd", ops.device_lr(groups[0], lrs[0]))     # (the group's device scalar while a whole-step graph captures: graph.py)
