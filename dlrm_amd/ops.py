"""Tensor-level wrappers around the C ABI (no autograd here; see functional.py).

Every function enqueues HIP kernels on torch's current stream for the tensors' device and returns
immediately.  Tensors must be fp32 CUDA(HIP) tensors whose last dimension is contiguous; leading
dimensions are passed as explicit strides so strided views (e.g. a slot of the [B, F, D] interaction
buffer) are used in place.  Anything else raises — there is no CPU/eager fallback.
"""
from __future__ import annotations

import os
import time

import ctypes as C
from typing import Callable, List, NamedTuple, Optional, Sequence, Union

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, UPD_ATOMIC, UPD_DETERMINISTIC, UPD_SORTED  # noqa: F401


def _stream(t: Optional[torch.Tensor] = None) -> C.c_void_p:
    """torch's current stream of the device the kernels will run on.  HIP launches go to the CURRENT device, so an operand
    that lives on another device (a model on cuda:1 in a process that never called torch.cuda.set_device(1)) is refused
    loudly instead of launching device-0 kernels on device-1 pointers."""
    if t is not None and t.is_cuda and t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"dlrm_amd: operand on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "call torch.cuda.set_device(...) (one process per GPU) before using the model")
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimers:
    """Optional HIP-event timing of the C-ABI launches, on the stream they are enqueued on (bench.py turns it on inside its
    timed region; None by default).

    One event is recorded where the launch CATEGORY changes (e.g. linear_fwd -> emb_fwd), not around every launch: a run of
    consecutive launches of one category on one stream is a single (start, end) pair, and the end of one run is the start
    of the next.  Event records are not free on this hardware — each is a barrier packet, ~5 us of idle queue: two per
    launch cost 0.33 ms of a 9.1 ms step (rocprofv3 trace, profiles/r03/ceilings.md) and inflated every per-kernel time
    by 10 us — so this keeps ~35 of them per step instead of 120.  A run's time covers whatever the stream executed
    between its first launch and the next category's first launch: `mark()` closes the open run early wherever something
    that is not a kernel of this library follows (a collective, a cross-stream wait)."""

    def __init__(self):
        self.records = {}          # name -> {"calls": launches, "pairs": [(start_event, end_event), ...]}
        self._enabled = True       # bench.py samples a subset of its timed steps
        self._open = None          # [name, start_event, torch stream, launches]

    @property
    def enabled(self):
        return self._enabled

    @enabled.setter
    def enabled(self, on):
        if not on:
            self.mark()
        self._enabled = bool(on)

    def _close(self, end_event):
        name, start, _, calls = self._open
        rec = self.records.setdefault(name, {"calls": 0, "pairs": []})
        rec["calls"] += calls
        rec["pairs"].append((start, end_event))
        self._open = None

    def mark(self):
        """close the open run now (its end event is recorded on the stream the run was launched on)"""
        if self._open is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(self._open[2])
            self._close(e)

    def enter(self, name):
        if not self._enabled:
            return
        st = torch.cuda.current_stream()
        o = self._open
        if o is not None and o[2] == st:
            if o[0] == name:
                o[3] += 1
                return
            e = torch.cuda.Event(enable_timing=True)
            e.record(st)
            self._close(e)                       # shared: end of the previous run == start of this one
        else:
            self.mark()                          # a run on another stream ends with an event of its own
            e = torch.cuda.Event(enable_timing=True)
            e.record(st)
        self._open = [name, e, st, 1]

    def summary(self):
        self.mark()
        torch.cuda.synchronize()
        out = {}
        for name, rec in self.records.items():
            total = float(sum(a.elapsed_time(b) for a, b in rec["pairs"]))
            out[name] = {"calls": rec["calls"], "total_ms": total, "avg_ms": total / max(rec["calls"], 1)}
        return out


timers: Optional[KernelTimers] = None


def timer_mark() -> None:
    """called by code that enqueues non-library work (collectives, cross-stream waits): ends the open timing run"""
    if timers is not None:
        timers.mark()


CALL_COUNT = [0]      # categorised C-ABI calls since import (bench.py reports calls per step for the launch-bound workload)


class _timed:
    __slots__ = ("name",)

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        CALL_COUNT[0] += 1
        if timers is not None:
            timers.enter(self.name)
        return self

    def __exit__(self, *exc):
        return False


def _req(t: torch.Tensor, name: str, dtype=torch.float32, ndim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"dlrm_amd: `{name}` must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"dlrm_amd: `{name}` must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"dlrm_amd: `{name}` must be {ndim}-D, got shape {tuple(t.shape)}")
    if t.dim() >= 1 and t.numel() > 0 and t.stride(-1) != 1:
        raise RuntimeError(f"dlrm_amd: `{name}` must be contiguous in its last dimension")


def _ld(t: torch.Tensor) -> int:
    """leading dimension (elements) of a 2-D row-major view"""
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


# ------------------------------------------------------------------------------------------------
# out-of-range embedding indices
# ------------------------------------------------------------------------------------------------
_err_blocks = {}   # device index -> pinned host int64[4] the embedding kernels report into (include/dlrm_hip.h, `err`)


def _err_block(device: torch.device) -> torch.Tensor:
    """Pinned host memory is device-visible under HIP's unified addressing: the kernels store {1, table, index, rows}
    straight into it when they meet an index outside [0, rows), and the host polls it WITHOUT synchronising."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    blk = _err_blocks.get(key)
    if blk is None:
        blk = torch.zeros(4, dtype=torch.int64).pin_memory()
        _err_blocks[key] = blk
    return blk


def check_index_errors(device=None, sync: bool = False) -> None:
    """Raise IndexError if an embedding kernel that has FINISHED met an out-of-range index (the lookup was skipped on the
    device; the reference's EmbeddingBag raises at the call).  sync=True first waits for the device, which makes the
    check exact for everything enqueued so far; without it the check costs one host memory read (DLRM_Net.forward does
    that at every step, so bad data is reported at most one step late)."""
    if sync and torch.cuda.is_available():
        torch.cuda.synchronize(device)
    for key, blk in _err_blocks.items():
        if device is not None and torch.device(device).index not in (None, key):
            continue
        if int(blk[0]) != 0:
            _, t, idx, rows = blk.tolist()
            blk.zero_()
            if rows == -1:
                raise IndexError(f"dlrm_amd: the fused one-lookup-per-bag embedding + interaction path met a bag of table {t} that "
                                 f"does not start at its own position (offset {-idx - 1}); set model.fuse_emb_interact = False for "
                                 f"multi-hot / ragged batches (cuda:{key})")
            raise IndexError(f"dlrm_amd: embedding index out of range: table {t}, index {idx}, rows {rows} (cuda:{key})")


# ------------------------------------------------------------------------------------------------
# embedding bags
# ------------------------------------------------------------------------------------------------
class BagBatch:
    """Host-side descriptor of one batch of bags for T tables (device pointers + sizes).

    Mirrors what `apply_emb` receives (dlrm_s_pytorch.py:407): lS_o[k] = bag starts of table k,
    lS_i[k] = flat indices of table k; both either lists of 1-D tensors or stacked 2-D tensors."""

    def __init__(self, lS_o, lS_i, per_sample_weights: Optional[Sequence[Optional[torch.Tensor]]] = None):
        T = len(lS_i)
        if len(lS_o) != T:
            raise RuntimeError("dlrm_amd: offsets / indices table counts differ")
        self.T = T
        self.ignore_oob = False   # True: out-of-range ids are expected (row-wise shards: ids of other ranks' rows) — skipped, not reported
        self.keep = []  # keep tensors alive while kernels may still read them
        if isinstance(lS_i, torch.Tensor) and isinstance(lS_o, torch.Tensor) and lS_i.dim() == 2 and lS_o.dim() == 2:
            # stacked [T, n] inputs (what the reference's collate functions build, dlrm_data_pytorch.py:686,337): the
            # per-table pointers are plain address arithmetic — no 2*T view tensors per step on the host path
            if lS_i.dtype not in (torch.int64, torch.int32) or lS_o.dtype != lS_i.dtype:
                raise RuntimeError("dlrm_amd: indices/offsets must both be int64 or both int32")
            if not lS_i.is_cuda or not lS_o.is_cuda:
                raise RuntimeError("dlrm_amd: indices/offsets must be GPU tensors")
            if lS_i.stride(1) != 1 and lS_i.size(1) > 1:
                lS_i = lS_i.contiguous()
            if lS_o.stride(1) != 1 and lS_o.size(1) > 1:
                lS_o = lS_o.contiguous()
            self.keep += [lS_i, lS_o]
            isz = lS_i.element_size()
            B, n_i = lS_o.size(1), lS_i.size(1)
            dt = lS_i.dtype
            idx_ptrs = [lS_i.data_ptr() + k * lS_i.stride(0) * isz if n_i else 0 for k in range(T)]
            off_ptrs = [lS_o.data_ptr() + k * lS_o.stride(0) * isz for k in range(T)]
            nnz = [n_i] * T
            self._idx_src = lS_i
            self._off_src = lS_o
        else:
            idx_ptrs, off_ptrs, nnz = [], [], []
            dt = None
            B = None
            self._idx_src = []
            self._off_src = []
            for k in range(T):
                i_k, o_k = lS_i[k], lS_o[k]
                if i_k.dtype not in (torch.int64, torch.int32) or o_k.dtype != i_k.dtype:
                    raise RuntimeError("dlrm_amd: indices/offsets must both be int64 or both int32")
                if dt is None:
                    dt = i_k.dtype
                elif dt != i_k.dtype:
                    raise RuntimeError("dlrm_amd: all tables must use the same index dtype")
                if not i_k.is_cuda or not o_k.is_cuda:
                    raise RuntimeError("dlrm_amd: indices/offsets must be GPU tensors")
                if not i_k.is_contiguous():
                    i_k = i_k.contiguous()
                if not o_k.is_contiguous():
                    o_k = o_k.contiguous()
                if B is None:
                    B = o_k.numel()
                elif B != o_k.numel():
                    raise RuntimeError("dlrm_amd: every table must have the same number of bags")
                self.keep += [i_k, o_k]
                self._idx_src.append(i_k)
                self._off_src.append(o_k)
                idx_ptrs.append(i_k.data_ptr() if i_k.numel() else 0)
                off_ptrs.append(o_k.data_ptr())
                nnz.append(i_k.numel())
        self.B = int(B)
        self.idx_bits = 64 if dt == torch.int64 else 32
        self.nnz = nnz
        self._idx = _lib.ptr_array(idx_ptrs)
        self._off = _lib.ptr_array(off_ptrs)
        self._nnz = _lib.i64_array(nnz)
        self._psw = None
        if per_sample_weights is not None and any(w is not None for w in per_sample_weights):
            ptrs = []
            for k, w in enumerate(per_sample_weights):
                if w is None:
                    ptrs.append(0)
                else:
                    _req(w, "per_sample_weights")
                    if w.numel() != nnz[k]:
                        raise RuntimeError("dlrm_amd: per_sample_weights size mismatch")
                    w = w.contiguous()
                    self.keep.append(w)
                    ptrs.append(w.data_ptr())
            self._psw = _lib.ptr_array(ptrs)


def pool_weights_gather(vws: Sequence[torch.Tensor], bags: "BagBatch") -> List[torch.Tensor]:
    """psw[t][i] = vws[t][idx_t[i]] (`v_W_l[k].gather(0, indices)`, dlrm_s_pytorch.py:425-426) for all tables in one launch;
    attaches the result to `bags` as its per-sample weights."""
    lib = _lib.load()
    if len(vws) != bags.T:
        raise RuntimeError("dlrm_amd: pool_weights_gather needs one weight vector per table")
    for v in vws:
        _req(v, "pooling weights", ndim=1)
    dev = vws[0].device
    psw = [torch.empty(n, dtype=torch.float32, device=dev) for n in bags.nnz]
    rc = lib.dlrm_pool_weights_gather(bags.T, _lib.i64_array([v.numel() for v in vws]), bags._idx, bags._nnz, bags.idx_bits,
                                      _lib.ptr_array([v.data_ptr() for v in vws]),
                                      _lib.ptr_array([p_.data_ptr() if p_.numel() else 0 for p_ in psw]),
                                      C.c_void_p(_err_block(dev).data_ptr()), _stream(vws[0]))
    _lib.check(rc, "dlrm_pool_weights_gather")
    bags.keep += psw
    bags._psw = _lib.ptr_array([p_.data_ptr() if p_.numel() else 0 for p_ in psw])
    return psw


def emb_psw_grad(weights: Sequence[torch.Tensor], bags: "BagBatch", dout: torch.Tensor, like: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """dense gradients of the learned pooling-weight vectors: dvW_t[r] = sum_{lookups of row r} <dout[bag], W_t[r]>"""
    lib = _lib.load()
    D, wp, rows = _weights_desc(weights)
    _req(dout, "dout", ndim=2)
    dvw = [torch.empty_like(v) for v in like]
    rc = lib.dlrm_emb_psw_grad(bags.T, bags.B, D, wp, rows, bags._idx, bags._off, bags._nnz, bags.idx_bits,
                               C.c_void_p(dout.data_ptr()), _ld(dout), _lib.ptr_array([g.data_ptr() for g in dvw]), _stream(dout))
    _lib.check(rc, "dlrm_emb_psw_grad")
    return dvw


def bag_index_tensor(bags: "BagBatch", k: int) -> torch.Tensor:
    """the 1-D index tensor of table k as it was passed in (the COO gradient's indices, verbatim)"""
    return bags._idx_src[k]


def _weights_desc(weights: Sequence[torch.Tensor]):
    D = None
    for w in weights:
        _req(w, "embedding weight", ndim=2)
        if not w.is_contiguous():
            raise RuntimeError("dlrm_amd: embedding tables must be contiguous [rows, D]")
        if D is None:
            D = w.size(1)
        elif D != w.size(1):
            raise RuntimeError("dlrm_amd: all embedding tables must share one embedding dimension")
    return int(D), _lib.ptr_array([w.data_ptr() for w in weights]), _lib.i64_array([w.size(0) for w in weights])


def _pred_args(pred, stream: C.c_void_p):
    """pred = (flag, nonzero): flag a device int32 tensor; the launch runs iff (flag != 0) == bool(nonzero) (include/dlrm_hip.h, ABI 16).
    stream: what _stream() gave the launch.  A flag of iota.offsets_iota_state names the stream its pool was allocated under; used on
    another one it is recorded there, torch's convention for memory used off its allocating stream (dlrm_amd/iota.py, rule 3)."""
    flag, nonzero = pred
    if flag.dtype != torch.int32 or not flag.is_cuda or flag.numel() < 1:
        raise RuntimeError("dlrm_amd: a launch predicate is a device int32 tensor")
    home = getattr(flag, "dlrm_pool_stream", None)
    if home is not None and home != (stream.value or 0):
        flag.record_stream(torch.cuda.current_stream())
    return C.c_void_p(flag.data_ptr()), int(bool(nonzero))


def emb_fwd(weights: Sequence[torch.Tensor], bags: BagBatch, out: torch.Tensor, pred=None) -> torch.Tensor:
    """out[b, t*D:(t+1)*D] = sum-pooled bag (t, b).  `out` is a [B, >= T*D] view (row stride free).  pred: see _pred_args."""
    return _pooled_lookup("fp32", (weights,), bags, out, pred)


def quant_row_bytes(D: int, bits: int) -> int:
    """bytes of one packed row in torch's fused row-wise format: D codes + fp32 scale, bias (8 bits); D/2 + fp16 scale, bias (4 bits)"""
    if bits == 8:
        return int(D) + 8
    if bits == 4:
        if D % 2:
            raise RuntimeError("dlrm_amd: the 4-bit row format needs an even embedding dimension, got %d" % D)
        return int(D) // 2 + 4
    raise RuntimeError("dlrm_amd: quantised embedding rows have 4 or 8 bits, got %r" % (bits,))


def emb_quantize(weight: torch.Tensor, bits: int) -> torch.Tensor:
    """uint8 [rows, quant_row_bytes(D, bits)]: `weight` ([rows, D] fp32) in torch's fused row-wise format, byte for byte what
    `torch.ops.quantized.embedding_bag_{byte,4bit}_prepack` gives on the CPU (dlrm_s_pytorch.py:465-481), packed on the device."""
    _req(weight, "embedding weight", ndim=2)
    if not weight.is_contiguous():
        raise RuntimeError("dlrm_amd: embedding tables must be contiguous [rows, D]")
    rows, D = weight.shape
    out = torch.empty((rows, quant_row_bytes(D, bits)), dtype=torch.uint8, device=weight.device)
    if rows == 0:
        return out
    lib = _lib.load()
    with _timed("emb_quantize"):
        rc = lib.dlrm_emb_quantize_rows(rows, D, bits, C.c_void_p(weight.data_ptr()), C.c_void_p(out.data_ptr()), _stream(weight))
    _lib.check(rc, "dlrm_emb_quantize_rows")
    return out


def _packed_tables_desc(qweights: Sequence[torch.Tensor], rows: Sequence[int], D: int, bits: int, T: int, what: str):
    rb = quant_row_bytes(D, bits)
    if len(qweights) != T or len(rows) != T:
        raise RuntimeError("dlrm_amd: %s needs one packed table and one row count per table" % what)
    for q, n in zip(qweights, rows):
        _req(q, "packed embedding table", dtype=torch.uint8, ndim=2)
        if not q.is_contiguous() or q.size(0) != int(n) or q.size(1) != rb:
            raise RuntimeError("dlrm_amd: a packed %d-bit table of %d rows and dimension %d is a contiguous uint8 [%d, %d] tensor, got %s"
                               % (bits, n, D, n, rb, tuple(q.shape)))
    return _lib.ptr_array([q.data_ptr() for q in qweights]), _lib.i64_array(rows)


def _packed_rows_desc(qweights, rows, D, bits, T, what):
    return (D,) + _packed_tables_desc(qweights, rows, D, bits, T, what)


def emb_fwd_quant(qweights: Sequence[torch.Tensor], rows: Sequence[int], D: int, bits: int, bags: BagBatch, out: torch.Tensor,
                  pred=None) -> torch.Tensor:
    """emb_fwd over packed tables (emb_quantize): out[b, t*D:(t+1)*D] = sum_i psw_i * (scale_r * q_r + bias_r).  qweights[t] is the
    uint8 [rows[t], quant_row_bytes(D, bits)] tensor of table t; `out` is a [B, >= T*D] view (row stride free).  pred: see _pred_args."""
    return _pooled_lookup("quant", (qweights, rows, D, bits, bags.T, "emb_fwd_quant"), bags, out, pred, (bits,))


# ---- quotient-remainder (QR) tables: csrc/emb_qr.hip.  A table list is described by three parallel lists: `weights` (weight_q of a QR table,
# the table itself for a plain one), `weights_r` (weight_r or None), `rows` (the number of CATEGORIES n of a QR table — weight_q has
# ceil(n / c) rows —, the row count of a plain one) and `collisions` (c, 0 for a plain table).
QR_OPS = {"mult": _lib.QR_MULT, "add": _lib.QR_ADD}


def _qr_op(op) -> int:
    try:
        return QR_OPS[op]
    except KeyError:
        raise RuntimeError("dlrm_amd: the QR composition is 'mult' or 'add', got %r" % (op,)) from None


def _i32_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def qr_rows_q(n: int, collisions: int) -> int:
    """rows of weight_q: ceil(n / c) (qr_embedding_bag.py:155-158)"""
    return -(-int(n) // int(collisions))


def _qr_desc(weights, weights_r, rows, collisions):
    T = len(weights)
    if not (len(weights_r) == len(rows) == len(collisions) == T) or T == 0:
        raise RuntimeError("dlrm_amd: a QR table list needs one weight, weight_r (or None), row count and collision count per table")
    D = int(weights[0].size(1))
    for w, wr, n, c in zip(weights, weights_r, rows, collisions):
        _req(w, "embedding weight", ndim=2)
        want = (qr_rows_q(n, c) if c else int(n), D)
        if not w.is_contiguous() or tuple(w.shape) != want:
            raise RuntimeError("dlrm_amd: a table of %d rows with %d collisions needs a contiguous weight of shape %s, got %s" % (n, c, want, tuple(w.shape)))
        if c:
            _req(wr, "embedding weight_r", ndim=2)
            if not wr.is_contiguous() or tuple(wr.shape) != (int(c), D):
                raise RuntimeError("dlrm_amd: weight_r of a table with %d collisions is a contiguous [%d, %d] tensor, got %s" % (c, c, D, tuple(wr.shape)))
    return (D, _lib.ptr_array([w.data_ptr() for w in weights]), _lib.ptr_array([wr.data_ptr() if c else 0 for wr, c in zip(weights_r, collisions)]),
            _lib.i64_array(rows), _i32_array(collisions))


def emb_fwd_qr(weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]], rows: Sequence[int], collisions: Sequence[int],
               op: str, bags: BagBatch, out: torch.Tensor, saved: Optional[torch.Tensor] = None, pred=None) -> torch.Tensor:
    """emb_fwd over a table list with QR tables: out[b, t*D:(t+1)*D] = (sum Wq[q_i]) op (sum Wr[r_i]) for a QR table, the pooled sum for a plain
    one.  saved: a [B, >= 2*Tq*D] buffer that receives the two sums of every QR table (what emb_qr_bwd_split reads).
    pred = (flag, nonzero): launch predicate (dlrm_emb_fwd_qr_pred)."""
    lib = _lib.load()
    D, wp, wrp, rows_a, coll_a = _qr_desc(weights, weights_r, rows, collisions)
    _req(out, "out", ndim=2)
    if out.size(0) != bags.B or out.size(1) < bags.T * D or len(weights) != bags.T:
        raise RuntimeError("dlrm_amd: emb_fwd_qr shape mismatch")
    if bags._psw is not None:
        raise RuntimeError("dlrm_amd: QR tables take no per-sample (pooling) weights")
    sv_p, sv_ld = None, 0
    if saved is not None:
        _req(saved, "saved", ndim=2)
        if saved.size(0) != bags.B or saved.size(1) < 2 * D * sum(1 for c in collisions if c):
            raise RuntimeError("dlrm_amd: emb_fwd_qr `saved` is a [B, >= 2 * (QR tables) * D] buffer")
        sv_p, sv_ld = C.c_void_p(saved.data_ptr()), _ld(saved)
    err = None if bags.ignore_oob else C.c_void_p(_err_block(out.device).data_ptr())
    st = _stream(out)
    with _timed("emb_fwd" if pred is None else "emb_interact_fwd_qr"):
        if pred is None:
            rc = lib.dlrm_emb_fwd_qr(bags.T, bags.B, D, wp, wrp, rows_a, coll_a, _qr_op(op), bags._idx, bags._off, bags._nnz, bags.idx_bits,
                                     C.c_void_p(out.data_ptr()), _ld(out), sv_p, sv_ld, err, st)
        else:
            rc = lib.dlrm_emb_fwd_qr_pred(bags.T, bags.B, D, wp, wrp, rows_a, coll_a, _qr_op(op), bags._idx, bags._off, bags._nnz,
                                          bags.idx_bits, C.c_void_p(out.data_ptr()), _ld(out), sv_p, sv_ld, err, *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_emb_fwd_qr")
    return out


def emb_qr_bwd_split(collisions: Sequence[int], op: str, D: int, dout: torch.Tensor, saved: Optional[torch.Tensor],
                     gout: Optional[torch.Tensor] = None, pred=None) -> torch.Tensor:
    """[B, Tv*D] gradient buffer of the virtual table list (a QR table = its q table, then its r table) from dout [B, >= T*D]:
    dout * sr, dout * sq ("mult"; `saved` of emb_fwd_qr) | dout, dout ("add") | a copy for plain tables.
    pred = (flag, nonzero): launch predicate (dlrm_emb_qr_bwd_split_pred)."""
    lib = _lib.load()
    T = len(collisions)
    Tv = T + sum(1 for c in collisions if c)
    _req(dout, "dout", ndim=2)
    if dout.size(1) < T * D:
        raise RuntimeError("dlrm_amd: emb_qr_bwd_split shape mismatch")
    B = dout.size(0)
    if gout is None:
        gout = torch.empty((B, Tv * D), dtype=torch.float32, device=dout.device)
    _req(gout, "gout", ndim=2)
    if gout.size(0) != B or gout.size(1) < Tv * D:
        raise RuntimeError("dlrm_amd: emb_qr_bwd_split needs a [B, >= Tv*D] output")
    sv_p, sv_ld = None, 0
    if saved is not None:
        _req(saved, "saved", ndim=2)
        if saved.size(0) != B or saved.size(1) < 2 * D * (Tv - T):
            raise RuntimeError("dlrm_amd: emb_qr_bwd_split `saved` is a [B, >= 2 * (QR tables) * D] buffer")
        sv_p, sv_ld = C.c_void_p(saved.data_ptr()), _ld(saved)
    st = _stream(dout)
    with _timed("emb_qr_bwd_split" if pred is None else "emb_interact_bwd_qr"):
        if pred is None:
            rc = lib.dlrm_emb_qr_bwd_split(T, B, D, _i32_array(collisions), _qr_op(op), C.c_void_p(dout.data_ptr()), _ld(dout), sv_p, sv_ld,
                                           C.c_void_p(gout.data_ptr()), _ld(gout), st)
        else:
            rc = lib.dlrm_emb_qr_bwd_split_pred(T, B, D, _i32_array(collisions), _qr_op(op), C.c_void_p(dout.data_ptr()), _ld(dout), sv_p,
                                                sv_ld, C.c_void_p(gout.data_ptr()), _ld(gout), *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_emb_qr_bwd_split")
    return gout


def emb_qr_split_indices(rows: Sequence[int], collisions: Sequence[int], bags: BagBatch):
    """(q ids, r ids) per table — None, None for a plain table — in the dtype of the ids; q = (id / c).long() with the reference's float32
    division, r = id mod c; -1 / -1 for a lookup the forward skips."""
    lib = _lib.load()
    if len(rows) != bags.T or len(collisions) != bags.T:
        raise RuntimeError("dlrm_amd: emb_qr_split_indices needs one row count and one collision count per table")
    ks = [k for k, c in enumerate(collisions) if c]
    qs, rs = [None] * bags.T, [None] * bags.T
    if not ks:
        return qs, rs
    src = [bag_index_tensor(bags, k) for k in ks]
    for k, i_k in zip(ks, src):
        qs[k], rs[k] = torch.empty_like(i_k), torch.empty_like(i_k)
    with _timed("emb_qr_split_indices"):
        rc = lib.dlrm_emb_qr_split_indices(len(ks), _lib.i64_array([rows[k] for k in ks]), _i32_array([collisions[k] for k in ks]),
                                           _lib.ptr_array([i_k.data_ptr() if i_k.numel() else 0 for i_k in src]),
                                           _lib.i64_array([i_k.numel() for i_k in src]), bags.idx_bits,
                                           _lib.ptr_array([qs[k].data_ptr() if qs[k].numel() else 0 for k in ks]),
                                           _lib.ptr_array([rs[k].data_ptr() if rs[k].numel() else 0 for k in ks]), _stream(src[0]))
    _lib.check(rc, "dlrm_emb_qr_split_indices")
    return qs, rs


def qr_virtual_bags(rows: Sequence[int], collisions: Sequence[int], bags: BagBatch) -> BagBatch:
    """The bags of the virtual table list: a QR table becomes two plain tables (its q ids, then its r ids) that share its bag offsets; a
    plain table stays one.  What the sparse updates (emb_bwd_sgd, emb_bwd_coo, ...) take together with emb_qr_bwd_split's buffer."""
    qs, rs = emb_qr_split_indices(rows, collisions, bags)
    lS_o, lS_i = [], []
    for k, c in enumerate(collisions):
        off, idx = bags._off_src[k], bag_index_tensor(bags, k)
        if c:
            lS_o += [off, off]
            lS_i += [qs[k], rs[k]]
        else:
            lS_o.append(off)
            lS_i.append(idx)
    vb = BagBatch(lS_o, lS_i, None)
    vb.ignore_oob = bags.ignore_oob
    return vb


# ---- mixed-dimension (MD) tables: csrc/emb_md.hip.  Table t is `weights[t]` [rows_t, d_t] with its own width and `projs[t]`, the [D, d_t] weight
# of a bias-free nn.Linear(d_t, D), or None (nn.Identity: d_t == D).
def alpha_power_rule(n: torch.Tensor, alpha: float, d0=None, B=None) -> torch.Tensor:
    """d_k = lambda * n_k^-alpha over the SORTED row counts `n` (float32 arithmetic, as tricks/md_embedding_bag.py:45-58): lambda =
    d0 * n_0^alpha (the smallest table keeps d0) or B / sum n^(1 - alpha) (parameter budget); never below 1; rounded half to even."""
    n = n.to(torch.float32)
    if d0 is not None:
        lamb = d0 * n[0] ** alpha
    elif B is not None:
        lamb = B / torch.sum(n ** (1 - alpha))
    else:
        raise ValueError("Must specify either d0 or B")
    d = torch.ones(len(n)) * lamb * n ** (-alpha)
    d = torch.where(d < 1, torch.ones_like(d), d)
    if d0 is not None:
        d[0] = d0
    return torch.round(d).to(torch.long)


def pow_2_round(dims: torch.Tensor) -> torch.Tensor:
    """the nearest power of two in log scale (md_embedding_bag.py:61-62); an integer tensor here (the reference returns floats)"""
    return (2 ** torch.round(torch.log2(dims.to(torch.float32)))).to(torch.long)


def md_solver(n, alpha: float, d0=None, B=None, round_dim: bool = True, k=None) -> torch.Tensor:
    """Per-table embedding widths of the mixed-dimension trick (md_embedding_bag.py:22-42; dlrm_s_pytorch.py:1213-1219 calls it with the table
    sizes, --md-temperature, d0 = --arch-sparse-feature-size and --md-round-dims), in the order of `n`.  Returns an int64 tensor."""
    n = torch.as_tensor(n)
    n_sorted, order = torch.sort(n)
    kk = k[order] if k is not None else torch.ones(len(n))
    d = alpha_power_rule(n_sorted.to(torch.float32) / kk, alpha, d0=d0, B=B)
    if round_dim:
        d = pow_2_round(d)
    out = torch.empty_like(d)
    out[order] = d
    return out


class MDLayout:
    """Columns of the pooled sums (`saved`) and of their gradients (`gout`) for per-table widths `dims`: tables of equal width are contiguous,
    widths descending, every group starts at a multiple of 4 floats.  cols[t]: first column of table t; groups: (d, [tables], first column) —
    gout[:, c0 : c0 + len(tables) * d] is the [B, n * d] gradient buffer of the group's tables for the sparse updates; width: columns in all
    (a multiple of 4)."""

    def __init__(self, dims: Sequence[int]):
        self.dims = [int(d) for d in dims]
        self.cols = [0] * len(self.dims)
        self.groups = []
        c = 0
        for d in sorted(set(self.dims), reverse=True):
            ks = [t for t, dt in enumerate(self.dims) if dt == d]
            self.groups.append((d, ks, c))
            for i, t in enumerate(ks):
                self.cols[t] = c + i * d
            c = (c + len(ks) * d + 3) // 4 * 4
        self.width = max(c, 4)


def bag_subset(bags: BagBatch, ks: Sequence[int]) -> BagBatch:
    """the bags of tables `ks` (one width group of an MD table list) as a BagBatch of their own"""
    sub = BagBatch([bags._off_src[k] for k in ks], [bags._idx_src[k] for k in ks], None)
    sub.ignore_oob = bags.ignore_oob
    return sub


def _md_desc(weights, projs, D):
    T = len(weights)
    if T == 0 or len(projs) != T:
        raise RuntimeError("dlrm_amd: an MD table list needs one weight and one projection (or None) per table")
    dims = []
    for w, p_ in zip(weights, projs):
        _req(w, "embedding weight", ndim=2)
        if not w.is_contiguous():
            raise RuntimeError("dlrm_amd: embedding tables must be contiguous [rows, d]")
        d = int(w.size(1))
        if p_ is None:
            if d != D:
                raise RuntimeError("dlrm_amd: an MD table without projection must have the common width %d, got %d" % (D, d))
        else:
            _req(p_, "projection weight", ndim=2)
            if not p_.is_contiguous() or tuple(p_.shape) != (D, d):
                raise RuntimeError("dlrm_amd: the projection of a table of width %d is a contiguous [%d, %d] tensor, got %s" % (d, D, d, tuple(p_.shape)))
        dims.append(d)
    return dims


def emb_fwd_md(weights: Sequence[torch.Tensor], projs: Sequence[Optional[torch.Tensor]], D: int, bags: BagBatch, out: torch.Tensor,
               saved: Optional[torch.Tensor] = None, cols: Optional[Sequence[int]] = None) -> torch.Tensor:
    """out[b, t*D:(t+1)*D] = (sum-pooled bag (t, b) of weights[t]) @ projs[t].T (projs[t] None: the pooled bag itself) for all tables in one launch.
    `out` is a [B, >= T*D] view (row stride free).  saved + cols (MDLayout.cols): the pooled sums go to saved[:, cols[t] : cols[t] + d_t]."""
    lib = _lib.load()
    D = int(D)
    dims = _md_desc(weights, projs, D)
    _req(out, "out", ndim=2)
    if out.size(0) != bags.B or out.size(1) < bags.T * D or len(weights) != bags.T:
        raise RuntimeError("dlrm_amd: emb_fwd_md shape mismatch")
    if bags._psw is not None:
        raise RuntimeError("dlrm_amd: MD tables take no per-sample (pooling) weights")
    sv_p, sv_ld, col_a = None, 0, None
    if saved is not None:
        _req(saved, "saved", ndim=2)
        if cols is None or len(cols) != bags.T or saved.size(0) != bags.B or any(c < 0 or c + d > saved.size(1) for c, d in zip(cols, dims)):
            raise RuntimeError("dlrm_amd: emb_fwd_md `saved` is a [B, >= max(cols[t] + d_t)] buffer with one first column per table")
        sv_p, sv_ld, col_a = C.c_void_p(saved.data_ptr()), _ld(saved), _i32_array(cols)
    err = None if bags.ignore_oob else C.c_void_p(_err_block(out.device).data_ptr())
    with _timed("emb_fwd"):
        rc = lib.dlrm_emb_fwd_md(bags.T, bags.B, D, _i32_array(dims), _lib.ptr_array([w.data_ptr() for w in weights]),
                                 _lib.ptr_array([p_.data_ptr() if p_ is not None else 0 for p_ in projs]),
                                 _lib.i64_array([w.size(0) for w in weights]), bags._idx, bags._off, bags._nnz, bags.idx_bits,
                                 C.c_void_p(out.data_ptr()), _ld(out), sv_p, sv_ld, col_a, err, _stream(out))
    _lib.check(rc, "dlrm_emb_fwd_md")
    return out


def emb_md_bwd(projs: Sequence[Optional[torch.Tensor]], dims: Sequence[int], D: int, dout: torch.Tensor, saved: Optional[torch.Tensor],
               cols: Sequence[int], gout: torch.Tensor, want_dproj: Optional[Sequence[bool]] = None):
    """Backward of emb_fwd_md in one call: gout[:, cols[t] : cols[t] + d_t] = dout[:, t*D:(t+1)*D] @ projs[t] (a copy for an identity table) and, for
    every projected table with want_dproj[t] (default: all), dproj[t] = dout[:, t*D:(t+1)*D].T @ saved[:, cols[t] : cols[t] + d_t] — a fresh [D, d_t]
    tensor, deterministic.  Returns (gout, [dproj or None per table])."""
    lib = _lib.load()
    T, D = len(projs), int(D)
    _req(dout, "dout", ndim=2)
    _req(gout, "gout", ndim=2)
    B = dout.size(0)
    if len(dims) != T or len(cols) != T or dout.size(1) < T * D or gout.size(0) != B or any(c < 0 or c + d > gout.size(1) for c, d in zip(cols, dims)):
        raise RuntimeError("dlrm_amd: emb_md_bwd shape mismatch")
    want = [p_ is not None and (want_dproj is None or bool(want_dproj[t])) for t, p_ in enumerate(projs)]
    dprojs = [torch.empty((D, int(d)), dtype=torch.float32, device=dout.device) if w_ else None for d, w_ in zip(dims, want)]
    sv_p, sv_ld, ws_p, ws_n = None, 0, None, 0
    if any(want):
        if saved is None:
            raise RuntimeError("dlrm_amd: this MD lookup ran without gradients enabled; its pooled sums were not kept")
        _req(saved, "saved", ndim=2)
        if saved.size(0) != B or any(c + d > saved.size(1) for c, d in zip(cols, dims)):
            raise RuntimeError("dlrm_amd: emb_md_bwd `saved` is the [B, >= max(cols[t] + d_t)] buffer emb_fwd_md filled")
        sv_p, sv_ld = C.c_void_p(saved.data_ptr()), _ld(saved)
        need = lib.dlrm_emb_md_bwd_workspace_bytes(T, B, D, _i32_array(dims))
        if need < 0:
            raise RuntimeError("dlrm_amd: dlrm_emb_md_bwd_workspace_bytes failed")
        ws = _scratch("md", need, dout.device)
        ws_p, ws_n = C.c_void_p(ws.data_ptr()), ws.numel()
    with _timed("emb_md_bwd"):
        rc = lib.dlrm_emb_md_bwd(T, B, D, _i32_array(dims), _lib.ptr_array([p_.data_ptr() if p_ is not None else 0 for p_ in projs]),
                                 C.c_void_p(dout.data_ptr()), _ld(dout), sv_p, sv_ld, _i32_array(cols), C.c_void_p(gout.data_ptr()), _ld(gout),
                                 _lib.ptr_array([g.data_ptr() if g is not None else 0 for g in dprojs]), ws_p, ws_n, _stream(dout))
    _lib.check(rc, "dlrm_emb_md_bwd")
    return gout, dprojs


_scratch_ws = {}   # (kind, device, stream) -> cached uint8 scratch: "emb" the workspace of the sort-based updates, "wgrad" the split-K slabs
                   # of the weight gradients, "tower" the slabs of tower_wgrad, "md" the slab partials of emb_md_bwd.  Per stream: kernels of
                   # one stream are ordered, so one buffer per kind suffices — and a buffer allocated under one stream is never handed to kernels of another (the caching allocator
                   # orders re-use of freed memory within the allocating stream only).  Grow-only; GraphedTrainStep pins what a capture used.


def _scratch(kind: str, need: int, device, stream: Optional[int] = None) -> Optional[torch.Tensor]:
    """stream: the handle of the stream of the TENSORS' device the launch uses (default: its current stream)"""
    if kind == "wgrad" and need <= 0:
        return None                      # (no split-K for this shape: linear_head_bwd takes it as "outside the fast path")
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream if stream is None else stream)
    ws = _scratch_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _scratch_ws[key] = torch.empty(max(int(need), 256) if kind == "emb" else int(need), dtype=torch.uint8, device=device)
    return ws


def _emb_sort_bytes(lib, bags: "BagBatch", rows) -> int:
    need = lib.dlrm_emb_bwd_workspace_bytes(bags.T, bags._nnz, rows)
    if need < 0:
        raise RuntimeError("dlrm_amd: dlrm_emb_bwd_workspace_bytes failed")
    return need


def sort_is_graph_safe(weights: Sequence[torch.Tensor], bags: BagBatch) -> bool:
    """True when the sort-based embedding updates of these shapes run entirely on the library's own segmented sorter
    (csrc/seg_sort.h: plain kernels, replayable inside a HIP graph); False when a table segment needs the general sorter."""
    if len(weights) != bags.T:
        raise RuntimeError("dlrm_amd: sort_is_graph_safe needs one table per bag list")
    desc = _bf16_weights_desc if weights and weights[0].dtype == torch.bfloat16 else _weights_desc      # (one sorter under every walk)
    _, _, rows = desc(weights)
    return _lib.load().dlrm_emb_sort_kind(bags.T, bags._nnz, rows) == 1


def sort_lookups(rows: Sequence[int], bags: BagBatch):
    """The (table, row) sort of the sort-based updates on its own (dlrm_emb_sort_lookups; bags.T <= 32): returns
    (positions uint32-as-int64 [L], keys int64 [L] = table << row_bits | row, bag_of int64 [L] (-1: skipped lookup), row_bits)."""
    lib = _lib.load()
    dev = bags.keep[0].device
    rows_a = _lib.i64_array([int(r) for r in rows])
    ws = _scratch("emb", _emb_sort_bytes(lib, bags, rows_a), dev)
    L = int(sum(bags.nnz))
    pos = torch.empty(L, dtype=torch.int32, device=dev)
    keys = torch.empty(L, dtype=torch.int64, device=dev)
    bag_of = torch.empty(L, dtype=torch.int32, device=dev)
    rb = C.c_int(0)
    rc = lib.dlrm_emb_sort_lookups(bags.T, bags.B, rows_a, bags._idx, bags._off, bags._nnz, bags.idx_bits, C.c_void_p(ws.data_ptr()),
                                   ws.numel(), C.c_void_p(pos.data_ptr()), C.c_void_p(keys.data_ptr()), C.c_void_p(bag_of.data_ptr()),
                                   C.byref(rb), C.c_void_p(_err_block(dev).data_ptr()), _stream(pos))
    _lib.check(rc, "dlrm_emb_sort_lookups")
    return pos.long() & 0xFFFFFFFF, keys, bag_of.long(), rb.value


# ---- learning rates: a Python float (by value in the launch) or a 1-element fp32 GPU tensor the kernel reads WHEN IT RUNS (include/dlrm_hip.h,
# "LEARNING RATES").  The second form is what a captured whole-step HIP graph takes, so that the reference's per-iteration LRPolicyScheduler
# (dlrm_s_pytorch.py:169-203, stepped at :1621) is followed without re-capture: GraphedTrainStep registers one device scalar per param group for
# the duration of the capture, the optimizer-side callers ask device_lr(group, value) for it.
# the bf16-shaped GEMM kernels (csrc/gemm_bf16.hip) are what the product library runs wherever their preconditions hold; the fp32-shaped
# ones can only be forced in a TUNING build of the library (DLRM_HIP_LIB=... DLRM_BF16_PHASED=0: tools/bf16_gemm_bench.py), and only then does
# the host plan follow the switch
BF16_PHASED = not (os.environ.get("DLRM_HIP_LIB") and os.environ.get("DLRM_BF16_PHASED", "1") == "0")

LrLike = Union[float, torch.Tensor]
_graph_lr = {}          # id(param_group dict) -> 1-element fp32 GPU tensor; populated only while a GraphedTrainStep captures


def device_lr(group, value):
    """the device scalar registered for this param group (inside a graph capture), else `value` unchanged"""
    t = _graph_lr.get(id(group))
    return t if t is not None else value


def _lr_args(lr: LrLike):
    if isinstance(lr, torch.Tensor):
        if lr.dtype != torch.float32 or not lr.is_cuda or lr.numel() != 1:
            raise RuntimeError("dlrm_amd: a device-side learning rate must be a 1-element float32 GPU tensor")
        return 0.0, C.c_void_p(lr.data_ptr())
    return float(lr), None


def _check_dout(name: str, dout: torch.Tensor, bags: BagBatch, D: int, *per_table) -> None:
    """what every sparse update refuses first: `dout` is a [B, >= T*D] buffer, and every list of `per_table` has one entry per table"""
    _req(dout, "dout", ndim=2)
    if dout.size(0) != bags.B or dout.size(1) < bags.T * D or any(len(l) != bags.T for l in per_table):
        raise RuntimeError("dlrm_amd: %s shape mismatch" % name)


class Presorted:
    """What dlrm_emb_presort left behind for one backward pass: the workspace holding the lookups sorted by (table, row), the per-sample
    mask of SINGLE lookups (bit t of mask[b]: lookup (t, b) is the only one of the batch naming its row), the step size both update calls
    use and the launch predicate the fused backward ran under (None: unconditional)."""

    __slots__ = ("ws", "mask", "lr", "pred")

    def __init__(self, ws, mask, lr, pred):
        self.ws, self.mask, self.lr, self.pred = ws, mask, lr, pred


def presort_ok(weights: Sequence[torch.Tensor], bags: BagBatch) -> bool:
    """shapes dlrm_emb_presort / dlrm_emb_bwd_sgd_presorted take: one launch group, one lookup per bag position, D = 128, no pooling weights"""
    return (0 < bags.T <= 32 and len(weights) == bags.T and all(n == bags.B for n in bags.nnz) and bags._psw is None
            and all(w.size(1) == 128 and w.is_contiguous() and w.data_ptr() % 16 == 0 for w in weights))


def emb_presort(weights: Sequence[torch.Tensor], bags: BagBatch, lr: LrLike, pred=None) -> Presorted:
    """The sort of the sparse update, IN FRONT of the fused backward (dlrm_emb_presort, ABI 17): a fresh workspace (it must survive until
    emb_bwd_sgd_presorted consumes it, whatever else sorts in between) + the mask of single lookups."""
    lib = _lib.load()
    D, wp, rows = _weights_desc(weights)
    dev = weights[0].device
    ws = torch.empty(max(_emb_sort_bytes(lib, bags, rows), 256), dtype=torch.uint8, device=dev)
    mask = torch.empty(bags.B, dtype=torch.int32, device=dev)
    with _timed("emb_bwd_sgd"):
        rc = lib.dlrm_emb_presort(bags.T, bags.B, rows, bags._idx, bags._off, bags._nnz, bags.idx_bits, C.c_void_p(ws.data_ptr()), ws.numel(),
                                  C.c_void_p(mask.data_ptr()), None if bags.ignore_oob else C.c_void_p(_err_block(dev).data_ptr()), _stream(mask))
    _lib.check(rc, "dlrm_emb_presort")
    return Presorted(ws, mask, lr, pred)


def emb_bwd_sgd_presorted(weights: Sequence[torch.Tensor], bags: BagBatch, dout: torch.Tensor, pre: Presorted, skip_singles: bool = True) -> None:
    """The second half of emb_bwd_sgd(UPD_SORTED) from a Presorted workspace; skip_singles: the lookups the fused backward already applied
    (interact_bwd_gather(..., presorted=pre)) are left out — when the launch predicate it ran under holds."""
    lib = _lib.load()
    D, wp, rows = _weights_desc(weights)
    _check_dout("emb_bwd_sgd_presorted", dout, bags, D, weights)
    lr_v, lr_p = _lr_args(pre.lr)
    st = _stream(dout)
    flag, nz = _pred_args(pre.pred, st) if pre.pred is not None else (None, 0)
    with _timed("emb_bwd_sgd"):
        rc = lib.dlrm_emb_bwd_sgd_presorted(bags.T, bags.B, D, wp, rows, bags._nnz, C.c_void_p(dout.data_ptr()), _ld(dout), lr_v, lr_p,
                                            C.c_void_p(pre.ws.data_ptr()), pre.ws.numel(), int(bool(skip_singles)), flag, nz, st)
    _lib.check(rc, "dlrm_emb_bwd_sgd_presorted")


# ---- bfloat16 embedding tables: csrc/emb_bf16.hip.  Tables are torch.bfloat16 [rows, D]; the feature buffer, the gradient, the Adagrad
# accumulators and every sum stay fp32.  An update rounds each touched row ONCE: "nearest" (even) or "stochastic" (Philox4x32-10 keyed by
# `seed`: the same seed gives the same bits; the host restatement is tests/test_bf16_emb_host.py).
# `seed` is a Python int (the key travels by value in the launch) or a 1-element int64 GPU tensor holding the key's 64 bits, which the kernels
# read WHEN THEY RUN (the *_devkey calls, include/dlrm_hip.h "STEP STATE ON THE DEVICE") — the form a captured whole-step graph takes, as
# LrLike is for step sizes: GraphedTrainStep(device_step_state=True) registers a DeviceStepState per model for the duration of the capture,
# DLRM_Net._run_update then draws its keys with philox_key_next instead of on the host.
BF16_ROUNDINGS = {"nearest": 0, "stochastic": 1}
SeedLike = Union[int, torch.Tensor]


class DeviceStepState:
    """(calls, key): the number of bf16 update calls so far and the Philox key of the current one, both on the device (one int64 [2] tensor);
    draws / passes: keys drawn and parked backward passes applied while it was registered (what the capture is checked against)."""

    __slots__ = ("buf", "calls", "key", "draws", "passes")

    def __init__(self, calls: int, device):
        self.buf = torch.tensor([int(calls), 0], dtype=torch.int64, device=device)
        self.calls, self.key = self.buf[0:1], self.buf[1:2]
        self.draws = self.passes = 0


_graph_step_state = {}   # id(model) -> DeviceStepState; populated only while a GraphedTrainStep(device_step_state=True) captures


def device_step_state(model):
    """the device step state registered for this model (inside a graph capture), else None"""
    return _graph_step_state.get(id(model))


def _seed_args(seed: SeedLike):
    """(True, pointer) for a device-side key, (False, the 64 bits) for a host one"""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or not seed.is_cuda or seed.numel() != 1:
            raise RuntimeError("dlrm_amd: a device-side bf16 rounding seed must be a 1-element int64 GPU tensor")
        return True, C.c_void_p(seed.data_ptr())
    return False, int(seed) & (2 ** 64 - 1)


def philox_key_next(seed0: int, calls: torch.Tensor, key: torch.Tensor) -> None:
    """key[0] = _mix_seed(seed0, calls[0]) (dlrm_net), then calls[0] += 1, on the device in stream order (dlrm_philox_key_next: one tiny
    launch, nothing allocated, nothing synchronised).  calls, key: distinct 1-element int64 GPU tensors (the key's 64 bits as stored)."""
    for t, name in ((calls, "calls"), (key, "key")):
        _req(t, name, dtype=torch.int64)
        if t.numel() != 1:
            raise RuntimeError("dlrm_amd: philox_key_next takes 1-element int64 GPU tensors")
    if calls.device != key.device or calls.data_ptr() == key.data_ptr():
        raise RuntimeError("dlrm_amd: philox_key_next needs distinct tensors on one device")
    rc = _lib.load().dlrm_philox_key_next(int(seed0) & (2 ** 64 - 1), C.c_void_p(calls.data_ptr()), C.c_void_p(key.data_ptr()), _stream(key))
    _lib.check(rc, "dlrm_philox_key_next")


def _bf16_rounding(rounding) -> int:
    if rounding not in BF16_ROUNDINGS:
        raise RuntimeError("dlrm_amd: bf16 table rounding is 'nearest' or 'stochastic', got %r" % (rounding,))
    return BF16_ROUNDINGS[rounding]


def _bf16_weights_desc(weights: Sequence[torch.Tensor]):
    D = None
    for w in weights:
        _req(w, "bf16 embedding weight", dtype=torch.bfloat16, ndim=2)
        if not w.is_contiguous():
            raise RuntimeError("dlrm_amd: embedding tables must be contiguous [rows, D]")
        if D is None:
            D = w.size(1)
        elif D != w.size(1):
            raise RuntimeError("dlrm_amd: all embedding tables must share one embedding dimension")
    return int(D), _lib.ptr_array([w.data_ptr() for w in weights]), _lib.i64_array([w.size(0) for w in weights])


def emb_fwd_bf16(weights: Sequence[torch.Tensor], bags: BagBatch, out: torch.Tensor, pred=None) -> torch.Tensor:
    """emb_fwd over torch.bfloat16 tables: out[b, t*D:(t+1)*D] = sum-pooled bag (t, b) in fp32, bit-identical to emb_fwd on the tables
    upcast to fp32.  `out` is an fp32 [B, >= T*D] view (row stride free).  pred: see _pred_args."""
    return _pooled_lookup("bf16", (weights,), bags, out, pred)


# ---- the pooled lookup of the two-kernel form.  The C calls of the plain tables of either dtype and of the packed ones share ONE argument list
#     (T, B, D, [bits,] <the tables>, idx, off, nnz, psw, idx_bits, out, ld, err, [flag, nonzero,] stream)
# so there is one wrapper (_pooled_lookup) over LOOKUP_KINDS, in the form of ROW_KINDS below: `tables` is the argument list of the kind's
# descriptor, the entries hold finished strings, the descriptor is called without a frame in between.  emb_fwd_qr and emb_fwd_md are NOT kinds
# of it: each has a `saved` buffer, a second table list (weight_r, the projections) and refusals of its own — folding them in would add
# parameters to the wrapper, not remove code.
class LookupKind(NamedTuple):
    fwd: str                # the C symbols: unconditional, and behind a launch predicate (_pred_args)
    fwd_pred: str
    timer: str              # the timer categories: a predicated launch belongs to the step's fused lookup + interaction (one run with it)
    timer_pred: str
    desc: Callable          # desc(*tables) -> (D, then the ctypes arguments between `D, [bits]` and `idx`)


LOOKUP_KINDS = {
    "fp32": LookupKind("dlrm_emb_fwd", "dlrm_emb_fwd_pred", "emb_fwd", "emb_interact_fwd", _weights_desc),
    "bf16": LookupKind("dlrm_emb_fwd_bf16", "dlrm_emb_fwd_bf16_pred", "emb_fwd_bf16", "emb_interact_fwd_bf16", _bf16_weights_desc),
    "quant": LookupKind("dlrm_emb_fwd_quant", "dlrm_emb_fwd_quant_pred", "emb_fwd_quant", "emb_interact_fwd_quant", _packed_rows_desc),
}


def _pooled_lookup(kind: str, tables, bags: BagBatch, out: torch.Tensor, pred, lead=()) -> torch.Tensor:
    """out[b, t*D:(t+1)*D] = sum-pooled bag (t, b) of the tables of `kind`.  lead: the scalars behind D (packed: bits)."""
    k = LOOKUP_KINDS[kind]
    lib = _lib.load()
    d = k.desc(*tables)
    D = d[0]
    _req(out, "out", ndim=2)
    if out.size(0) != bags.B or out.size(1) < bags.T * D or len(tables[0]) != bags.T:
        raise RuntimeError("dlrm_amd: %s shape mismatch" % k.fwd[5:])
    err = None if bags.ignore_oob else C.c_void_p(_err_block(out.device).data_ptr())
    st = _stream(out)
    fn, timer, tail = (k.fwd, k.timer, (st,)) if pred is None else (k.fwd_pred, k.timer_pred, (*_pred_args(pred, st), st))
    with _timed(timer):
        rc = getattr(lib, fn)(bags.T, bags.B, D, *lead, *d[1:], bags._idx, bags._off, bags._nnz, bags._psw, bags.idx_bits,
                              C.c_void_p(out.data_ptr()), _ld(out), err, *tail)
    _lib.check(rc, k.fwd)
    return out


# ---- the sparse updates: fused EmbeddingBag backward + optimizer step, in place.  Below them is one device body (walk_update in
# csrc/sorted_walk.h, which takes a row-update policy); their C calls share ONE argument list
#     (T, B, D, tables, [states,] rows, idx, off, nnz, psw, idx_bits, dout, ld, lr, lr_dev, [eps,] [mode | rounding, seed, table0,] ws, ws_bytes, err, stream)
# so there is one wrapper (_sparse_update) over UPDATE_KINDS, which holds what differs.  dlrm_emb_presort and dlrm_emb_bwd_sgd_presorted above
# take other lists and keep their own calls.
class UpdateKind(NamedTuple):
    fn: str                 # the C symbol; without "dlrm_", the public wrapper's name in "<name> shape mismatch"
    timer: str              # the timer category
    desc: Callable          # _weights_desc | _bf16_weights_desc
    ws: str                 # the C symbol that sizes the workspace
    acc: Optional[str]      # the accumulators in `states`: None, "rows" ([rows] per table) or "table" (the table's shape)
    eps: bool               # the extra scalars, in the order of the list above: eps;
    mode: bool              # the UPD_* mode (only UPD_SORTED takes a workspace: that of the sort alone, sized without D);
    rounding: bool          # rounding, seed, table0


UPDATE_KINDS = {
    "sgd": UpdateKind("dlrm_emb_bwd_sgd", "emb_bwd_sgd", _weights_desc, "dlrm_emb_bwd_workspace_bytes", None, False, True, False),
    "rwsadagrad": UpdateKind("dlrm_emb_bwd_rowwise_adagrad", "emb_bwd_adagrad", _weights_desc, "dlrm_emb_adagrad_workspace_bytes", "rows",
                             True, False, False),
    "adagrad": UpdateKind("dlrm_emb_bwd_adagrad", "emb_bwd_adagrad", _weights_desc, "dlrm_emb_adagrad_workspace_bytes", "table",
                          True, False, False),
    "sgd_bf16": UpdateKind("dlrm_emb_bwd_sgd_bf16", "emb_bwd_sgd_bf16", _bf16_weights_desc, "dlrm_emb_bwd_bf16_workspace_bytes", None,
                           False, False, True),
    "rwsadagrad_bf16": UpdateKind("dlrm_emb_bwd_rowwise_adagrad_bf16", "emb_bwd_adagrad_bf16", _bf16_weights_desc,
                                  "dlrm_emb_bwd_bf16_workspace_bytes", "rows", True, False, True),
}


def _sparse_update(kind: str, weights, bags: BagBatch, dout: torch.Tensor, lr: LrLike, states=None, eps=None, mode=None, rounding=None,
                   seed: SeedLike = 0, table0: int = 0) -> None:
    """the update of `kind` over one backward pass (the public wrappers below say what each computes); states: the accumulators, one per table"""
    k = UPDATE_KINDS[kind]
    lib = _lib.load()
    D, wp, rows = k.desc(weights)
    if k.acc is None:
        _check_dout(k.fn[5:], dout, bags, D, weights)
        tables = (wp,)
    else:
        _check_dout(k.fn[5:], dout, bags, D, weights, states)
        for s_, w in zip(states, weights):
            if k.acc == "rows":
                _req(s_, "adagrad state", ndim=1)
                if s_.numel() != w.size(0) or not s_.is_contiguous():
                    raise RuntimeError("dlrm_amd: row-wise adagrad state must be a contiguous [rows] tensor")
            else:
                # (the kernel writes sums[t][row, 0:D] for every looked-up row: any other layout is an out-of-bounds device write)
                _req(s_, "adagrad sum", ndim=2)
                if tuple(s_.shape) != tuple(w.shape) or not s_.is_contiguous() or s_.device != w.device:
                    raise RuntimeError("dlrm_amd: adagrad sum must be a contiguous [rows, D] tensor on its table's device")
        tables = (wp, _lib.ptr_array([s_.data_ptr() for s_ in states]))
    extra = (float(eps),) if k.eps else ()
    fn = k.fn
    if k.mode:
        extra += (int(mode),)
    if k.rounding:
        on_device, seed_arg = _seed_args(seed)
        if on_device:
            fn += "_devkey"
        extra += (_bf16_rounding(rounding), seed_arg, int(table0))
    ws_ptr, ws_bytes = None, 0
    if not k.mode or mode == UPD_SORTED:
        need = getattr(lib, k.ws)(bags.T, bags._nnz, rows) if k.mode else getattr(lib, k.ws)(bags.T, D, bags._nnz, rows)
        if need < 0:
            raise RuntimeError("dlrm_amd: %s failed" % k.ws)
        ws = _scratch("emb", need, dout.device)
        ws_ptr, ws_bytes = C.c_void_p(ws.data_ptr()), ws.numel()
    lr_v, lr_p = _lr_args(lr)
    err = None if bags.ignore_oob else C.c_void_p(_err_block(dout.device).data_ptr())
    with _timed(k.timer):
        rc = getattr(lib, fn)(bags.T, bags.B, D, *tables, rows, bags._idx, bags._off, bags._nnz, bags._psw, bags.idx_bits,
                              C.c_void_p(dout.data_ptr()), _ld(dout), lr_v, lr_p, *extra, ws_ptr, ws_bytes, err, _stream(dout))
    _lib.check(rc, fn)


def emb_bwd_sgd(weights: Sequence[torch.Tensor], bags: BagBatch, dout: torch.Tensor, lr: LrLike,
                mode: int = UPD_SORTED) -> None:
    """Fused EmbeddingBag backward + sparse SGD: W_t[idx] -= lr * dout[bag, t*D:(t+1)*D] (in place)."""
    _sparse_update("sgd", weights, bags, dout, lr, mode=mode)


def emb_bwd_rowwise_adagrad(weights: Sequence[torch.Tensor], states: Sequence[torch.Tensor], bags: BagBatch,
                            dout: torch.Tensor, lr: LrLike, eps: float) -> None:
    """Fused EmbeddingBag backward + row-wise sparse Adagrad (optim/rwsadagrad.py:117-143), in place:
    per touched row r:  g_r = sum of its lookups' gradients;  states[t][r] += mean(g_r^2);
    W_t[r] -= lr * g_r / (sqrt(states[t][r]) + eps).  `lr` is the decayed clr of rwsadagrad.py:115."""
    _sparse_update("rwsadagrad", weights, bags, dout, lr, states, eps)


def emb_bwd_adagrad(weights: Sequence[torch.Tensor], sums: Sequence[torch.Tensor], bags: BagBatch,
                    dout: torch.Tensor, lr: LrLike, eps: float) -> None:
    """Fused EmbeddingBag backward + exact sparse Adagrad (torch.optim.Adagrad's sparse branch, the reference's --optimizer=adagrad), in
    place: per touched row r:  g_r = sum of its lookups' gradients (the order and bits of emb_bwd_rowwise_adagrad);
    sums[t][r] += g_r^2;  W_t[r] -= lr * g_r / (sqrt(sums[t][r]) + eps), per element.  `sums[t]` is torch's state["sum"] of table t:
    fp32, contiguous, the shape of the table.  `lr` is the decayed clr."""
    _sparse_update("adagrad", weights, bags, dout, lr, sums, eps)


def emb_bwd_sgd_bf16(weights: Sequence[torch.Tensor], bags: BagBatch, dout: torch.Tensor, lr: LrLike, rounding: str = "stochastic",
                     seed: SeedLike = 0, table0: int = 0) -> None:
    """Fused EmbeddingBag backward + sparse SGD over torch.bfloat16 tables, in place: per touched row r, g_r = the fp32 sum of its lookups'
    gradients (sorted walk, deterministic), W[r] = round(fmaf(-lr, g_r, float(W[r]))) — one rounding per row per call.  table0: index of
    weights[0] in the caller's full table list (the random stream of a table does not depend on how the list is cut into calls).  seed: the
    Philox key, an int or a 1-element int64 GPU tensor read when the kernels run (SeedLike above): the same key, the same bits."""
    _sparse_update("sgd_bf16", weights, bags, dout, lr, rounding=rounding, seed=seed, table0=table0)


def emb_bwd_rowwise_adagrad_bf16(weights: Sequence[torch.Tensor], states: Sequence[torch.Tensor], bags: BagBatch, dout: torch.Tensor,
                                 lr: LrLike, eps: float, rounding: str = "stochastic", seed: SeedLike = 0, table0: int = 0) -> None:
    """emb_bwd_rowwise_adagrad over torch.bfloat16 tables, in place.  `states` stay fp32 and receive the bits emb_bwd_rowwise_adagrad gives
    them on the upcast tables; W[r] = round(fmaf(-lr, g_r / (sqrt(states[t][r]) + eps), float(W[r]))), one rounding per row per call."""
    _sparse_update("rwsadagrad_bf16", weights, bags, dout, lr, states, eps, None, rounding, seed, table0)


def emb_bwd_coo(bags: BagBatch, dout: torch.Tensor, D: int) -> List[torch.Tensor]:
    """The reference's EmbeddingBag backward WITHOUT the fused update: per table the [nnz_t, D] value block of the sparse
    COO gradient (values[i] = psw[i] * dout[bag(i), t*D:(t+1)*D]; its indices are the lookup indices verbatim)."""
    lib = _lib.load()
    _req(dout, "dout", ndim=2)
    if dout.size(0) != bags.B or dout.size(1) < bags.T * D:
        raise RuntimeError("dlrm_amd: emb_bwd_coo shape mismatch")
    values = [torch.empty((n, D), dtype=torch.float32, device=dout.device) for n in bags.nnz]
    with _timed("emb_bwd_coo"):
        rc = lib.dlrm_emb_bwd_coo(bags.T, bags.B, D, bags._off, bags._nnz, bags._psw, bags.idx_bits,
                                  C.c_void_p(dout.data_ptr()), _ld(dout),
                                  _lib.ptr_array([v.data_ptr() if v.numel() else 0 for v in values]), _stream())
    _lib.check(rc, "dlrm_emb_bwd_coo")
    return values


# ------------------------------------------------------------------------------------------------
# interaction
# ------------------------------------------------------------------------------------------------
def _feature_table(tensors: Sequence[torch.Tensor], D: int):
    """Each [B, k*D] tensor contributes k features: (ptr + j*D*4, row stride)."""
    ptrs, lds = [], []
    B = tensors[0].size(0)
    for t in tensors:
        _req(t, "feature block", ndim=2)
        if t.size(0) != B or t.size(1) % D != 0:
            raise RuntimeError("dlrm_amd: feature blocks must be [B, k*D]")
        for j in range(t.size(1) // D):
            ptrs.append(t.data_ptr() + 4 * j * D)
            lds.append(_ld(t))
    return B, ptrs, lds


def interact_out_width(F: int, D: int, self_interaction) -> int:
    """self_interaction: False/0 = strictly lower triangle (the reference's order), True/1 = with the diagonal, 2 = torchrec's
    torch.triu_indices(F, F, 1) order (same pairs as 0, permuted columns)"""
    return D + (F * (F + 1) // 2 if (int(self_interaction) & 1) else F * (F - 1) // 2)


def _permute(order, *lists):
    return lists if order is None else tuple([l[i] for i in order] for l in lists)


def interact_fwd(blocks: Sequence[torch.Tensor], D: int, self_interaction: bool, R: torch.Tensor, order=None, pred=None) -> torch.Tensor:
    """order: optional permutation — canonical feature f is the order[f]-th feature of the block list (lets the interaction read
    features that live in several buffers, e.g. all-to-all blocks of table-wise shards + the reduce-scatter block of row-wise
    ones, in global table order without copying them together)"""
    lib = _lib.load()
    B, ptrs, lds = _feature_table(blocks, D)
    ptrs, lds = _permute(order, ptrs, lds)
    _req(R, "R", ndim=2)
    F = len(ptrs)
    if R.size(0) != B or R.size(1) < interact_out_width(F, D, self_interaction):
        raise RuntimeError("dlrm_amd: interact_fwd output shape mismatch")
    st = _stream(R)
    with _timed("interact_fwd" if pred is None else "emb_interact_fwd"):
        if pred is None:
            rc = lib.dlrm_interact_fwd(B, F, D, _lib.ptr_array(ptrs), _lib.i64_array(lds), int(self_interaction),
                                       C.c_void_p(R.data_ptr()), _ld(R), st)
        else:
            rc = lib.dlrm_interact_fwd_pred(B, F, D, _lib.ptr_array(ptrs), _lib.i64_array(lds), None, None, None, 64, int(self_interaction),
                                            C.c_void_p(R.data_ptr()), _ld(R), None, *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_interact_fwd")
    return R


def gather_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_ok(F, D))


# Host wait for an event that ends the host's run-ahead once per step: POLL it (hipEventQuery) instead of sleeping on it.
# hipEventSynchronize blocks the thread in the driver, and how long the wake-up takes after the GPU signalled is the BOX's business
# (interrupt routing, CPU idle states, a runtime that polls with sleeps): measured 30-110 us per step on most MI355X boxes of the pool and
# 1.25 ms on one (profiles/round6/proof_wait.md: the same step 9.14 ms instead of 7.89, the GPU idle while the host slept — the verdict of the
# proof was there, the bottom tower long finished).  The wait is at most one training step long; after SPIN_WAIT_S the thread sleeps after all.
SPIN_WAIT_S = 0.0 if os.environ.get("DLRM_SPIN_WAIT", "1") == "0" else 0.05        # DLRM_SPIN_WAIT=0: sleep on the event (A/B)


def wait_spinning(ev, limit_s: Optional[float] = None) -> None:
    """ev: a torch.cuda.Event or a torch.cuda.Stream (both have query() / synchronize()); limit_s: how long to poll before sleeping after all"""
    if ev.query():
        return
    end = time.perf_counter() + (SPIN_WAIT_S if limit_s is None else (limit_s if SPIN_WAIT_S > 0 else 0.0))
    while not ev.query():
        if time.perf_counter() > end:
            ev.synchronize()
            return


def _gather_one_lookup(bags: BagBatch, tables: int) -> None:
    """what every fused lookup + interaction wrapper refuses first: the kernels fetch ONE row per bag and apply no pooling weight"""
    if bags.T != tables or bags.nnz.count(bags.B) != len(bags.nnz):       # (a list of ints: count() instead of a generator per call)
        raise RuntimeError("dlrm_amd: the fused embedding + interaction path needs exactly one lookup per bag")
    if bags._psw is not None:
        raise RuntimeError("dlrm_amd: the fused embedding + interaction path does not take per-sample weights")


def _gather_desc(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int):
    """feature 0 = the [B, D] block x, features 1..T = the tables addressed through the bags' indices"""
    _gather_one_lookup(bags, len(weights))
    _req(x, "x", ndim=2)
    ptrs = [x.data_ptr()] + [w.data_ptr() for w in weights]
    lds = [_ld(x)] + [D] * len(weights)
    F = len(ptrs)
    gidx = (C.c_void_p * F)(None, *[C.c_void_p(bags._idx[k]) for k in range(bags.T)])
    goff = (C.c_void_p * F)(None, *[C.c_void_p(bags._off[k]) for k in range(bags.T)])
    rows = _lib.i64_array([0] + [w.size(0) for w in weights])
    return F, _lib.ptr_array(ptrs), _lib.i64_array(lds), gidx, goff, rows


def _gather_tables_bf16(weights: Sequence[torch.Tensor], what: str) -> bool:
    """True: every table is torch.bfloat16 (the calls of csrc/interact_bf16.hip); False: none is; a mixture is refused"""
    n16 = sum(1 for w in weights if w.dtype == torch.bfloat16)
    if n16 not in (0, len(weights)):
        raise RuntimeError("dlrm_amd: %s takes tables of ONE dtype, all fp32 or all bfloat16" % what)
    return n16 > 0


# ---- fused lookup + interaction over every table kind but fp32 at D = 128: bf16 (csrc/interact_bf16.hip), fp32 / bf16 / packed rows of D = 16 /
# 32 / 64 (interact_narrow.hip, interact_narrow_rows.hip), QR at both widths (interact_qr.hip, interact_narrow_qr.hip), packed at D = 128
# (interact_quant.hip).  Their C calls share ONE argument list
#     (B, F, D, [bits,] x, ldx, <the tables>, idx, off, idx_bits, mode, R | dR, ld, [dx, ld, dE | gout, ld,] err, flag, nonzero, stream)
# and one set of refusals, so there is one forward and one backward wrapper (_fwd_gather_rows, _bwd_gather_rows) over ROW_KINDS, which holds
# what differs.  `tables` is the argument list of the kind's descriptor, the list of table tensors first; desc(*tables) checks the tables and
# returns (their embedding dimension, then the ctypes arguments between `x, ldx` and `idx, off`).  These calls are on the per-step host
# path: the entries hold finished strings and the descriptors are called without a frame in between.
def _qr_rows_desc(weights, weights_r, rows, collisions, op):
    return _qr_desc(weights, weights_r, rows, collisions) + (_qr_op(op),)


class RowKind(NamedTuple):
    fwd: str                # the C symbols; bwd None: forward only (packed tables are constants)
    bwd: Optional[str]
    timer_fwd: str          # the timer categories
    timer_bwd: Optional[str]
    desc: Callable          # see above
    word: str               # the kind in "the fused <word> embedding + interaction path: shape mismatch"
    align: int              # bytes a table's base address is a multiple of: one lane's load of a row (packed: of 8-bit rows; 4-bit rows half)


ROW_KINDS = {
    "bf16": RowKind("dlrm_interact_fwd_gather_bf16", "dlrm_interact_bwd_gather_bf16", "emb_interact_fwd_bf16", "emb_interact_bwd_bf16",
                    _bf16_weights_desc, "bf16", 16),
    "narrow": RowKind("dlrm_interact_fwd_gather_narrow", "dlrm_interact_bwd_gather_narrow", "emb_interact_fwd_narrow", "emb_interact_bwd_narrow",
                      _weights_desc, "narrow", 16),
    "narrow_bf16": RowKind("dlrm_interact_fwd_gather_narrow_bf16", "dlrm_interact_bwd_gather_narrow_bf16", "emb_interact_fwd_narrow_bf16",
                           "emb_interact_bwd_narrow_bf16", _bf16_weights_desc, "narrow bf16", 8),
    "qr": RowKind("dlrm_interact_fwd_gather_qr", "dlrm_interact_bwd_gather_qr", "emb_interact_fwd_qr", "emb_interact_bwd_qr",
                  _qr_rows_desc, "QR", 16),
    "narrow_qr": RowKind("dlrm_interact_fwd_gather_narrow_qr", "dlrm_interact_bwd_gather_narrow_qr", "emb_interact_fwd_narrow_qr",
                         "emb_interact_bwd_narrow_qr", _qr_rows_desc, "QR", 16),
    "quant": RowKind("dlrm_interact_fwd_gather_quant", None, "emb_interact_fwd_quant", None, _packed_rows_desc, "quantised", 8),
    "narrow_quant": RowKind("dlrm_interact_fwd_gather_narrow_quant", None, "emb_interact_fwd_narrow_quant", None, _packed_rows_desc,
                            "narrow quantised", 8),
}
GATHER_ALIGN = 16       # ... and of the fp32 D = 128 kernels (dlrm_interact_fwd_gather): a lane's 4 columns are one 16-byte load


def _fwd_gather_rows(kind: str, x: torch.Tensor, tables, bags: BagBatch, D: int, mode, R: torch.Tensor, pred, lead=()) -> torch.Tensor:
    """R = interaction of [x | one row per bag of the tables of `kind`]; table t is feature t + 1.  lead: the scalars in front of x (packed:
    bits).  pred: see _pred_args; None = (NULL, 0), the launch always runs."""
    k = ROW_KINDS[kind]
    lib = _lib.load()
    _gather_one_lookup(bags, len(tables[0]))
    _req(x, "x", ndim=2)
    d = k.desc(*tables)
    if d[0] != D or x.size(1) != D or x.size(0) != bags.B:
        raise RuntimeError("dlrm_amd: the fused %s embedding + interaction path: shape mismatch" % k.word)
    _req(R, "R", ndim=2)
    F = 1 + bags.T
    if R.size(0) != bags.B or R.size(1) < interact_out_width(F, D, mode):
        raise RuntimeError("dlrm_amd: %s shape mismatch" % k.fwd[5:])
    st = _stream(R)
    flag, nonzero = (None, 0) if pred is None else _pred_args(pred, st)
    with _timed(k.timer_fwd):
        rc = getattr(lib, k.fwd)(bags.B, F, D, *lead, C.c_void_p(x.data_ptr()), _ld(x), *d[1:], bags._idx, bags._off, bags.idx_bits,
                                 int(mode), C.c_void_p(R.data_ptr()), _ld(R), C.c_void_p(_err_block(R.device).data_ptr()), flag, nonzero, st)
    _lib.check(rc, k.fwd)
    return R


def _bwd_gather_rows(kind: str, x: torch.Tensor, tables, bags: BagBatch, D: int, mode, dR: torch.Tensor, dx: torch.Tensor, dE: torch.Tensor,
                     grad_tables: int, pred) -> None:
    """dx [B, D] = gradient of x; dE [B, >= grad_tables * D] = gradients of the gathered rows (QR: `gout`, the buffer of the VIRTUAL table
    list, grad_tables = its length).  `mode | INTERACT_RELU_X` as interact_bwd."""
    k = ROW_KINDS[kind]
    if k.bwd is None:
        raise RuntimeError("dlrm_amd: the fused %s embedding + interaction path is forward only" % k.word)
    lib = _lib.load()
    _gather_one_lookup(bags, len(tables[0]))
    _req(x, "x", ndim=2)
    d = k.desc(*tables)
    if d[0] != D or x.size(1) != D or x.size(0) != bags.B:
        raise RuntimeError("dlrm_amd: the fused %s embedding + interaction path: shape mismatch" % k.word)
    _req(dR, "dR", ndim=2); _req(dx, "dx", ndim=2); _req(dE, "dE | gout", ndim=2)
    if dR.size(0) != bags.B or dx.size(0) != bags.B or dE.size(0) != bags.B or dx.size(1) < D or dE.size(1) < grad_tables * D:
        raise RuntimeError("dlrm_amd: %s shape mismatch" % k.bwd[5:])
    st = _stream(dR)
    flag, nonzero = (None, 0) if pred is None else _pred_args(pred, st)
    with _timed(k.timer_bwd):
        rc = getattr(lib, k.bwd)(bags.B, 1 + bags.T, D, C.c_void_p(x.data_ptr()), _ld(x), *d[1:], bags._idx, bags._off, bags.idx_bits,
                                 int(mode), C.c_void_p(dR.data_ptr()), _ld(dR), C.c_void_p(dx.data_ptr()), _ld(dx),
                                 C.c_void_p(dE.data_ptr()), _ld(dE), C.c_void_p(_err_block(dR.device).data_ptr()), flag, nonzero, st)
    _lib.check(rc, k.bwd)


def tables_aligned(tensors, align: int) -> bool:
    """every table's base address a multiple of `align` bytes (RowKind.align, GATHER_ALIGN)"""
    return all(t.data_ptr() % align == 0 for t in tensors)


def gather_bf16_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_bf16_ok(int(F), int(D)))


def bf16_tables_aligned(weights: Sequence[torch.Tensor]) -> bool:
    """what the fused bf16 kernels need of the tables: a lane's 8 columns are one 16-byte load"""
    return tables_aligned(weights, ROW_KINDS["bf16"].align)


def interact_fwd_gather(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction: bool,
                        R: torch.Tensor, pred=None) -> torch.Tensor:
    """R = interaction of [x | one-hot embedding rows], the rows fetched by the kernel itself (no pooled-embedding buffer).
    Tables all fp32, or all torch.bfloat16 (dlrm_interact_fwd_gather_bf16: the bits of emb_fwd_bf16 + interact_fwd)."""
    if _gather_tables_bf16(weights, "interact_fwd_gather"):
        return _fwd_gather_rows("bf16", x, (weights,), bags, D, self_interaction, R, pred)
    lib = _lib.load()
    F, p, ld, gidx, goff, rows = _gather_desc(x, weights, bags, D)
    _req(R, "R", ndim=2)
    if R.size(0) != bags.B or x.size(0) != bags.B or R.size(1) < interact_out_width(F, D, self_interaction):
        raise RuntimeError("dlrm_amd: interact_fwd_gather shape mismatch")
    st = _stream(R)
    with _timed("emb_interact_fwd"):
        if pred is None:
            rc = lib.dlrm_interact_fwd_gather(bags.B, F, D, p, ld, gidx, goff, rows, bags.idx_bits, int(self_interaction),
                                              C.c_void_p(R.data_ptr()), _ld(R), C.c_void_p(_err_block(R.device).data_ptr()), st)
        else:
            rc = lib.dlrm_interact_fwd_pred(bags.B, F, D, p, ld, gidx, goff, rows, bags.idx_bits, int(self_interaction),
                                            C.c_void_p(R.data_ptr()), _ld(R), C.c_void_p(_err_block(R.device).data_ptr()),
                                            *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_interact_fwd_gather")
    return R


# ---- fused lookup + interaction over QR tables (csrc/interact_qr.hip); the table list is described as for emb_fwd_qr
def gather_qr_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_qr_ok(int(F), int(D)))


def qr_tables_aligned(weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]]) -> bool:
    """what the fused QR kernels need of weight_q / weight_r / plain tables: a lane's 4 columns are one 16-byte load"""
    return tables_aligned([*weights, *(wr for wr in weights_r if wr is not None)], ROW_KINDS["qr"].align)


def interact_fwd_gather_qr(x: torch.Tensor, weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]], rows: Sequence[int],
                           collisions: Sequence[int], op: str, bags: BagBatch, D: int, self_interaction, R: torch.Tensor,
                           pred=None) -> torch.Tensor:
    """R = interaction of [x | the composed rows of the tables], the rows fetched and composed by the kernel itself
    (dlrm_interact_fwd_gather_qr): the bits of emb_fwd_qr into a feature buffer + interact_fwd, without that buffer."""
    return _fwd_gather_rows("qr", x, (weights, weights_r, rows, collisions, op), bags, D, self_interaction, R, pred)


def interact_bwd_gather_qr(x: torch.Tensor, weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]], rows: Sequence[int],
                           collisions: Sequence[int], op: str, bags: BagBatch, D: int, self_interaction, dR: torch.Tensor,
                           dx: torch.Tensor, gout: torch.Tensor, pred=None) -> None:
    """dx [B, D] = gradient of x; gout [B, >= Tv*D] = the gradient buffer of the VIRTUAL table list, as emb_qr_bwd_split lays it out
    (dlrm_interact_bwd_gather_qr): the bits of interact_bwd over (x, the buffer emb_fwd_qr wrote) + emb_qr_bwd_split, without the pooled
    buffer, its gradient or the saved sums.  `self_interaction | INTERACT_RELU_X` as interact_bwd."""
    _bwd_gather_rows("qr", x, (weights, weights_r, rows, collisions, op), bags, D, self_interaction, dR, dx, gout,
                     bags.T + sum(1 for c in collisions if c), pred)


# ---- ... and over QR tables of D = 16 / 32 / 64 (csrc/interact_narrow_qr.hip: the narrow kernels over a QR row source)
def gather_narrow_qr_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_narrow_qr_ok(int(F), int(D)))


def interact_fwd_gather_narrow_qr(x: torch.Tensor, weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]],
                                  rows: Sequence[int], collisions: Sequence[int], op: str, bags: BagBatch, D: int, self_interaction,
                                  R: torch.Tensor, pred=None) -> torch.Tensor:
    """interact_fwd_gather_qr for tables of D = 16 / 32 / 64 (dlrm_interact_fwd_gather_narrow_qr): the bits of emb_fwd_qr into a feature
    buffer + interact_fwd, without that buffer."""
    return _fwd_gather_rows("narrow_qr", x, (weights, weights_r, rows, collisions, op), bags, D, self_interaction, R, pred)


def interact_bwd_gather_narrow_qr(x: torch.Tensor, weights: Sequence[torch.Tensor], weights_r: Sequence[Optional[torch.Tensor]],
                                  rows: Sequence[int], collisions: Sequence[int], op: str, bags: BagBatch, D: int, self_interaction,
                                  dR: torch.Tensor, dx: torch.Tensor, gout: torch.Tensor, pred=None) -> None:
    """interact_bwd_gather_qr for tables of D = 16 / 32 / 64 (dlrm_interact_bwd_gather_narrow_qr): dx and the gradient buffer of the
    VIRTUAL table list with the bits of interact_bwd over (x, the buffer emb_fwd_qr wrote) + emb_qr_bwd_split."""
    _bwd_gather_rows("narrow_qr", x, (weights, weights_r, rows, collisions, op), bags, D, self_interaction, dR, dx, gout,
                     bags.T + sum(1 for c in collisions if c), pred)


def gather_quant_ok(F: int, D: int, bits: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_quant_ok(int(F), int(D), int(bits)))


def packed_align(bits: int) -> int:
    """a lane's codes are one 8-byte (8 bits) / 4-byte (4 bits) load"""
    align = ROW_KINDS["quant"].align
    return align if bits == 8 else align // 2


def quant_tables_aligned(qweights: Sequence[torch.Tensor], bits: int) -> bool:
    """what interact_fwd_gather_quant needs of the packed tables: packed_align(bits)"""
    return tables_aligned(qweights, packed_align(bits))


def interact_fwd_gather_quant(x: torch.Tensor, qweights: Sequence[torch.Tensor], rows: Sequence[int], D: int, bits: int, bags: BagBatch,
                              self_interaction, R: torch.Tensor, pred=None) -> torch.Tensor:
    """R = interaction of [x | one-hot rows of the packed tables], the rows fetched and dequantised by the kernel itself
    (dlrm_interact_fwd_gather_quant): the bits of emb_fwd_quant into a feature buffer + interact_fwd, without that buffer.  Forward only."""
    return _fwd_gather_rows("quant", x, (qweights, rows, D, bits, bags.T, "interact_fwd_gather_quant"), bags, D, self_interaction, R, pred,
                            (bits,))


INTERACT_RELU_X = 4         # DLRM_INTERACT_RELU_X of include/dlrm_hip.h: OR-ed into the backward kernels' interaction mode


def interact_bwd_gather(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction: bool,
                        dR: torch.Tensor, dx: torch.Tensor, dE: torch.Tensor, pred=None, presorted: Optional["Presorted"] = None) -> None:
    """dx [B, D] = gradient of x; dE [B, T*D] = gradients of the T gathered rows (the dout of the fused embedding update).
    `self_interaction | INTERACT_RELU_X`: x is a ReLU output and dx comes back multiplied by [x > 0] (see interact_bwd).
    presorted (emb_presort): the sparse SGD step of the single lookups is taken here — their tables rows are UPDATED, their dE rows not
    written; emb_bwd_sgd_presorted applies the rest (dlrm_interact_bwd_gather_sgd, ABI 17)."""
    if _gather_tables_bf16(weights, "interact_bwd_gather"):
        # bf16 tables (dlrm_interact_bwd_gather_bf16): the bits of interact_bwd over (x, the buffer emb_fwd_bf16 wrote)
        if presorted is not None:
            raise RuntimeError("dlrm_amd: interact_bwd_gather: the update inside the backward (presorted) exists for fp32 tables only")
        return _bwd_gather_rows("bf16", x, (weights,), bags, D, self_interaction, dR, dx, dE, bags.T, pred)
    lib = _lib.load()
    F, p, ld, gidx, goff, rows = _gather_desc(x, weights, bags, D)
    _req(dR, "dR", ndim=2); _req(dx, "dx", ndim=2); _req(dE, "dE", ndim=2)
    dptrs = [dx.data_ptr()] + [dE.data_ptr() + 4 * k * D for k in range(bags.T)]
    dlds = [_ld(dx)] + [_ld(dE)] * bags.T
    st = _stream(dR)
    with _timed("emb_interact_bwd"):
        if presorted is not None:
            lr_v, lr_p = _lr_args(presorted.lr)
            flag, nz = _pred_args(pred, st) if pred is not None else (None, 0)
            rc = lib.dlrm_interact_bwd_gather_sgd(bags.B, F, D, p, ld, gidx, goff, rows, bags.idx_bits, int(self_interaction),
                                                  C.c_void_p(dR.data_ptr()), _ld(dR), _lib.ptr_array(dptrs), _lib.i64_array(dlds),
                                                  C.c_void_p(presorted.mask.data_ptr()), lr_v, lr_p,
                                                  C.c_void_p(_err_block(dR.device).data_ptr()), flag, nz, st)
        elif pred is None:
            rc = lib.dlrm_interact_bwd_gather(bags.B, F, D, p, ld, gidx, goff, rows, bags.idx_bits, int(self_interaction),
                                              C.c_void_p(dR.data_ptr()), _ld(dR), _lib.ptr_array(dptrs), _lib.i64_array(dlds),
                                              C.c_void_p(_err_block(dR.device).data_ptr()), st)
        else:
            rc = lib.dlrm_interact_bwd_pred(bags.B, F, D, p, ld, gidx, goff, rows, bags.idx_bits, int(self_interaction),
                                            C.c_void_p(dR.data_ptr()), _ld(dR), _lib.ptr_array(dptrs), _lib.i64_array(dlds),
                                            C.c_void_p(_err_block(dR.device).data_ptr()), *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_interact_bwd_gather")


# ---- fused lookup + interaction over plain fp32 tables of D = 16 / 32 / 64 (csrc/interact_narrow.hip).  Separate functions: interact_*_gather
# keep refusing every D != 128
def gather_narrow_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_narrow_ok(int(F), int(D)))


def interact_fwd_gather_narrow(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction,
                               R: torch.Tensor, pred=None) -> torch.Tensor:
    """R = interaction of [x | one-hot rows of the fp32 tables], D = 16 / 32 / 64, the rows fetched by the kernel itself
    (dlrm_interact_fwd_gather_narrow): the bits of emb_fwd into a feature buffer + interact_fwd, without that buffer."""
    return _fwd_gather_rows("narrow", x, (weights,), bags, D, self_interaction, R, pred)


def interact_bwd_gather_narrow(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction,
                               dR: torch.Tensor, dx: torch.Tensor, dE: torch.Tensor, pred=None) -> None:
    """dx [B, D] = gradient of x; dE [B, T*D] = gradients of the T gathered rows (dlrm_interact_bwd_gather_narrow): the bits of
    interact_bwd over (x, the buffer emb_fwd wrote).  `self_interaction | INTERACT_RELU_X` as interact_bwd."""
    _bwd_gather_rows("narrow", x, (weights,), bags, D, self_interaction, dR, dx, dE, bags.T, pred)


# ---- ... and over bfloat16 / packed tables of those widths (csrc/interact_narrow_rows.hip: the same kernels over another row source).
# Separate functions again: interact_*_gather (bf16) and interact_fwd_gather_quant keep refusing every D != 128
def gather_narrow_bf16_ok(F: int, D: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_narrow_bf16_ok(int(F), int(D)))


def gather_narrow_quant_ok(F: int, D: int, bits: int) -> bool:
    return bool(_lib.load().dlrm_interact_gather_narrow_quant_ok(int(F), int(D), int(bits)))


def narrow_bf16_tables_aligned(weights: Sequence[torch.Tensor]) -> bool:
    """what the narrow fused bf16 kernels need of the tables: a lane's 4 columns are one 8-byte load"""
    return tables_aligned(weights, ROW_KINDS["narrow_bf16"].align)


def interact_fwd_gather_narrow_bf16(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction,
                                    R: torch.Tensor, pred=None) -> torch.Tensor:
    """R = interaction of [x | one-hot rows of the bfloat16 tables], D = 16 / 32 / 64, the rows fetched and widened by the kernel itself
    (dlrm_interact_fwd_gather_narrow_bf16): the bits of emb_fwd_bf16 into a feature buffer + interact_fwd, without that buffer."""
    return _fwd_gather_rows("narrow_bf16", x, (weights,), bags, D, self_interaction, R, pred)


def interact_bwd_gather_narrow_bf16(x: torch.Tensor, weights: Sequence[torch.Tensor], bags: BagBatch, D: int, self_interaction,
                                    dR: torch.Tensor, dx: torch.Tensor, dE: torch.Tensor, pred=None) -> None:
    """dx [B, D] = gradient of x; dE [B, T*D] = fp32 gradients of the T gathered bfloat16 rows (dlrm_interact_bwd_gather_narrow_bf16): the
    bits of interact_bwd over (x, the buffer emb_fwd_bf16 wrote).  `self_interaction | INTERACT_RELU_X` as interact_bwd."""
    _bwd_gather_rows("narrow_bf16", x, (weights,), bags, D, self_interaction, dR, dx, dE, bags.T, pred)


def interact_fwd_gather_narrow_quant(x: torch.Tensor, qweights: Sequence[torch.Tensor], rows: Sequence[int], D: int, bits: int,
                                     bags: BagBatch, self_interaction, R: torch.Tensor, pred=None) -> torch.Tensor:
    """R = interaction of [x | one-hot rows of the packed tables], D = 16 / 32 / 64, the rows fetched and dequantised by the kernel itself
    (dlrm_interact_fwd_gather_narrow_quant): the bits of emb_fwd_quant into a feature buffer + interact_fwd, without that buffer.
    Forward only."""
    return _fwd_gather_rows("narrow_quant", x, (qweights, rows, D, bits, bags.T, "interact_fwd_gather_narrow_quant"), bags, D,
                            self_interaction, R, pred, (bits,))


def interact_bwd(blocks: Sequence[torch.Tensor], D: int, self_interaction: bool, dR: torch.Tensor,
                 dblocks: Sequence[torch.Tensor], order=None, pred=None) -> None:
    """`self_interaction` is the forward's mode, optionally OR-ed with INTERACT_RELU_X: feature 0 (the first D columns of blocks[0],
    the bottom tower's output) is then taken as a ReLU output and its gradient is multiplied by the derivative [feature 0 > 0] inside
    the kernel, which has the feature staged anyway — the tower's backward then starts without its act_bwd pass over [B, D]."""
    lib = _lib.load()
    B, ptrs, lds = _feature_table(blocks, D)
    B2, dptrs, dlds = _feature_table(dblocks, D)
    ptrs, lds, dptrs, dlds = _permute(order, ptrs, lds, dptrs, dlds)
    _req(dR, "dR", ndim=2)
    if B != B2 or len(ptrs) != len(dptrs) or dR.size(0) != B:
        raise RuntimeError("dlrm_amd: interact_bwd shape mismatch")
    F = len(ptrs)
    st = _stream(dR)
    with _timed("interact_bwd" if pred is None else "emb_interact_bwd"):
        if pred is None:
            rc = lib.dlrm_interact_bwd(B, F, D, _lib.ptr_array(ptrs), _lib.i64_array(lds), int(self_interaction),
                                       C.c_void_p(dR.data_ptr()), _ld(dR), _lib.ptr_array(dptrs), _lib.i64_array(dlds), st)
        else:
            rc = lib.dlrm_interact_bwd_pred(B, F, D, _lib.ptr_array(ptrs), _lib.i64_array(lds), None, None, None, 64, int(self_interaction),
                                            C.c_void_p(dR.data_ptr()), _ld(dR), _lib.ptr_array(dptrs), _lib.i64_array(dlds), None,
                                            *_pred_args(pred, st), st)
    _lib.check(rc, "dlrm_interact_bwd")


def _proj_dims(P1: torch.Tensor, P2: torch.Tensor, D: int):
    """(I1, I2) of the projected interaction's operands P1 [B, I1*D], P2 [B, D*I2]; (0, 0) where the widths are no multiple of D"""
    D = int(D)
    if D < 1 or P1.size(1) % D or P2.size(1) % D:
        return 0, 0
    return P1.size(1) // D, P2.size(1) // D


def proj_interact_fwd(x: torch.Tensor, P1: torch.Tensor, P2: torch.Tensor, D: int, R: torch.Tensor) -> torch.Tensor:
    """R = [x | (P1 viewed [B, I1, D]) . (P2 viewed [B, D, I2]) flattened row-major | zeros] (dlrm_proj_interact_fwd): x [B, D] may be a
    column slice of a wider buffer, R [B, >= D + I1*I2]; the columns beyond D + I1*I2 are zero-filled."""
    lib = _lib.load()
    for t, name in ((x, "x"), (P1, "P1"), (P2, "P2"), (R, "R")):
        _req(t, name, ndim=2)
    B = x.size(0)
    I1, I2 = _proj_dims(P1, P2, D)
    if I1 < 1 or I2 < 1 or x.size(1) != D or P1.size(0) != B or P2.size(0) != B or R.size(0) != B or R.size(1) < D + I1 * I2:
        raise RuntimeError("dlrm_amd: proj_interact_fwd shape mismatch")
    with _timed("proj_interact_fwd"):
        rc = lib.dlrm_proj_interact_fwd(B, D, I1, I2, C.c_void_p(x.data_ptr()), _ld(x), C.c_void_p(P1.data_ptr()), _ld(P1),
                                        C.c_void_p(P2.data_ptr()), _ld(P2), C.c_void_p(R.data_ptr()), _ld(R), _stream(R))
    _lib.check(rc, "dlrm_proj_interact_fwd")
    return R


def proj_interact_bwd(P1: torch.Tensor, P2: torch.Tensor, D: int, dR: torch.Tensor, dx: torch.Tensor, dP1: torch.Tensor,
                      dP2: torch.Tensor) -> None:
    """dx = dR[:, :D], dP1 = dZ . Bm^T, dP2 = A^T . dZ (dlrm_proj_interact_bwd): overwrites dx [B, D], dP1 [B, I1*D], dP2 [B, D*I2]"""
    lib = _lib.load()
    for t, name in ((P1, "P1"), (P2, "P2"), (dR, "dR"), (dx, "dx"), (dP1, "dP1"), (dP2, "dP2")):
        _req(t, name, ndim=2)
    B = P1.size(0)
    I1, I2 = _proj_dims(P1, P2, D)
    if (I1 < 1 or I2 < 1 or P2.size(0) != B or dR.size(0) != B or dR.size(1) < D + I1 * I2 or tuple(dx.shape) != (B, D)
            or dP1.shape != P1.shape or dP2.shape != P2.shape):
        raise RuntimeError("dlrm_amd: proj_interact_bwd shape mismatch")
    with _timed("proj_interact_bwd"):
        rc = lib.dlrm_proj_interact_bwd(B, D, I1, I2, C.c_void_p(P1.data_ptr()), _ld(P1), C.c_void_p(P2.data_ptr()), _ld(P2),
                                        C.c_void_p(dR.data_ptr()), _ld(dR), C.c_void_p(dx.data_ptr()), _ld(dx),
                                        C.c_void_p(dP1.data_ptr()), _ld(dP1), C.c_void_p(dP2.data_ptr()), _ld(dP2), _stream(dR))
    _lib.check(rc, "dlrm_proj_interact_bwd")


# ------------------------------------------------------------------------------------------------
# MLP layers
# ------------------------------------------------------------------------------------------------
ARITH_NAMES = {"f32": _lib.ARITH_F32, "bf16x6": _lib.ARITH_BF16X6, "bf16": _lib.ARITH_BF16}


def arith_code(arith) -> int:
    """MLP arithmetic as the C ABI's per-call argument.  "f32": native fp32 MFMA.  "bf16x6": fp32 operands split exactly into
    3 bf16 terms, 6 bf16 MFMA products, fp32 accumulation (fp32 round-off class, 2.7x the matrix rate).  "bf16": operands
    rounded to bf16, one bf16 MFMA per 16-k step, fp32 accumulation — the reduced-precision "bf16 MLP" of BASELINE.json
    configs[4] (NOT fp32-class).  There is no process-wide switch: the arithmetic belongs to the module (FusedMLP.arith)
    and travels with every call.  See include/dlrm_hip.h."""
    if isinstance(arith, int) and arith in ARITH_NAMES.values():
        return arith
    if arith not in ARITH_NAMES:
        raise RuntimeError(f"dlrm_amd: unknown MLP arithmetic {arith!r} (f32 | bf16x6 | bf16)")
    return ARITH_NAMES[arith]


def round_bf16_k(K: int) -> int:
    """reduction length a bf16 operand copy is padded to: a multiple of 64 from 64 up (the bf16-shaped kernel's k-tile), of 32 below"""
    return (K + 63) & ~63 if K >= 64 else (K + 31) & ~31


def relu_bits_alloc(M: int, N: int, device) -> torch.Tensor:
    """buffer for the ReLU sign bits of an [M, N] activation (one bit per element, include/dlrm_hip.h)"""
    return torch.empty(_lib.load().dlrm_relu_bits_bytes(M, N) // 8, dtype=torch.int64, device=device)


def linear_fwd(X: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], act: int, Y: torch.Tensor,
               arith=_lib.ARITH_F32, relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    _req(X, "X", ndim=2); _req(W, "W", ndim=2); _req(Y, "Y", ndim=2)
    M, K = X.shape
    N = W.size(0)
    if W.size(1) != K or Y.size(0) != M or Y.size(1) != N:
        raise RuntimeError(f"dlrm_amd: linear_fwd shape mismatch X{tuple(X.shape)} W{tuple(W.shape)} Y{tuple(Y.shape)}")
    if bias is not None:
        _req(bias, "bias", ndim=1)
    with _timed("linear_fwd"):
        rc = lib.dlrm_linear_fwd(M, N, K, C.c_void_p(X.data_ptr()), _ld(X), C.c_void_p(W.data_ptr()), _ld(W),
                                 C.c_void_p(bias.data_ptr()) if bias is not None else None, int(act),
                                 C.c_void_p(Y.data_ptr()), _ld(Y),
                                 C.c_void_p(relu_bits.data_ptr()) if relu_bits is not None else None, arith_code(arith), _stream(Y))
    _lib.check(rc, "dlrm_linear_fwd")
    return Y


# ---- dynamically quantised int8 layers for inference: csrc/gemm_q8.hip (the reference's --quantize-mlp-with-bit 8)
Q8_RANGE, Q8_QUANTIZE = 1, 2


def q8_k64(K: int) -> int:
    """reduction length of the int8 operands: K padded with zero codes to a multiple of 64"""
    return (int(K) + 63) & ~63


class Q8Weight:
    """a Linear weight packed by q8_pack_weight: `codes` int8 [N, q8_k64(K)], `scale` device float[2] = {s_w, 1 / s_w}"""
    __slots__ = ("codes", "scale", "N", "K")

    def __init__(self, codes, scale, N, K):
        self.codes, self.scale, self.N, self.K = codes, scale, int(N), int(K)


def q8_pack_weight(W: torch.Tensor) -> Q8Weight:
    """torch's per-tensor symmetric qint8 weight of a dynamic quantised Linear (scale and int_repr() exactly), packed on the device"""
    _req(W, "W", ndim=2)
    N, K = W.shape
    if N < 1 or K < 1:
        raise RuntimeError("dlrm_amd: q8_pack_weight needs a non-empty [N, K] weight")
    codes = torch.empty((N, q8_k64(K)), dtype=torch.int8, device=W.device)
    scale = torch.empty(2, dtype=torch.float32, device=W.device)
    with _timed("q8_pack_weight"):
        rc = _lib.load().dlrm_q8_pack_weight(N, K, C.c_void_p(W.data_ptr()), _ld(W), C.c_void_p(codes.data_ptr()),
                                             C.c_void_p(scale.data_ptr()), _stream(W))
    _lib.check(rc, "dlrm_q8_pack_weight")
    return Q8Weight(codes, scale, N, K)


def q8_quantize_act(X: torch.Tensor, K: Optional[int] = None, phases: int = Q8_RANGE | Q8_QUANTIZE, bufs=None):
    """(codes int8 [M, q8_k64(K)], qparams device float[4] = {s_x, zero point, 1 / s_x, 0}) of the dynamic per-tensor quantisation of
    X[:, :K] (K defaults to X's width; columns from K on are padding and never read).  The parameters stay on the device.
    `bufs` = (codes, qparams, workspace) of an earlier call reuses them (the measurement tool's phase split)."""
    _req(X, "X", ndim=2)
    M = X.size(0)
    K = X.size(1) if K is None else int(K)
    if M < 1 or K < 1 or K > X.size(1):
        raise RuntimeError(f"dlrm_amd: q8_quantize_act needs a non-empty input of at least K = {K} columns, got {tuple(X.shape)}")
    lib = _lib.load()
    nws = int(lib.dlrm_q8_workspace_bytes(M, K))
    if bufs is None:
        bufs = (torch.empty((M, q8_k64(K)), dtype=torch.int8, device=X.device), torch.empty(4, dtype=torch.float32, device=X.device),
                torch.empty(nws // 4, dtype=torch.float32, device=X.device))
    codes, qparams, ws = bufs
    with _timed("q8_quantize_act"):
        rc = lib.dlrm_q8_quantize_act(M, K, C.c_void_p(X.data_ptr()), _ld(X), C.c_void_p(codes.data_ptr()), C.c_void_p(qparams.data_ptr()),
                                      C.c_void_p(ws.data_ptr()), nws, int(phases), _stream(X))
    _lib.check(rc, "dlrm_q8_quantize_act")
    return codes, qparams, ws


def gemm_q8(codes: torch.Tensor, qparams: torch.Tensor, W: Q8Weight, bias: Optional[torch.Tensor], act: int, out: torch.Tensor) -> torch.Tensor:
    """out = act(float(codes . W.codes^T) * (s_x * s_w) + bias) on the int8 MFMA; `out` is a [M, N] view with a free row stride"""
    _req(codes, "codes", dtype=torch.int8, ndim=2); _req(out, "out", ndim=2); _req(qparams, "qparams", ndim=1)
    M = codes.size(0)
    if (not codes.is_contiguous() or codes.size(1) != W.codes.size(1) or out.size(0) != M or out.size(1) != W.N or qparams.numel() < 3
            or M < 1):
        raise RuntimeError(f"dlrm_amd: gemm_q8 shape mismatch codes{tuple(codes.shape)} W{tuple(W.codes.shape)} out{tuple(out.shape)}")
    if bias is not None:
        _req(bias, "bias", ndim=1)
        if bias.numel() != W.N:
            raise RuntimeError("dlrm_amd: gemm_q8 bias length mismatch")
    with _timed("gemm_q8"):
        rc = _lib.load().dlrm_gemm_q8(M, W.N, W.K, C.c_void_p(codes.data_ptr()), C.c_void_p(W.codes.data_ptr()),
                                      C.c_void_p(qparams.data_ptr()), C.c_void_p(W.scale.data_ptr()),
                                      C.c_void_p(bias.data_ptr()) if bias is not None else None, int(act), C.c_void_p(out.data_ptr()),
                                      _ld(out), _stream(out))
    _lib.check(rc, "dlrm_gemm_q8")
    return out


def linear_q8(X: torch.Tensor, W: Q8Weight, bias: Optional[torch.Tensor], act: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch's dynamic int8 Linear (+ activation) of X: quantise the input per tensor, int8 GEMM, dequantise + bias.  X may carry zero
    padding columns beyond W.K (the interaction's 480-wide output for K = 479): they are not read."""
    if X.dim() != 2 or X.size(1) < W.K or X.size(1) > ((W.K + 3) & ~3):
        raise RuntimeError("dlrm_amd: linear_q8 input width %s does not match the layer (%d)" % (tuple(X.shape), W.K))
    codes, qparams, _ = q8_quantize_act(X, W.K)
    if out is None:
        out = torch.empty((X.size(0), W.N), dtype=torch.float32, device=X.device)
    return gemm_q8(codes, qparams, W, bias, act, out)


def linear_bwd_data(dY: torch.Tensor, W: torch.Tensor, Xact: Optional[torch.Tensor], xact_kind: int,
                    dX: torch.Tensor, arith=_lib.ARITH_F32, relu_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX = (dY @ W) * act'(Xact)   (Xact None -> no mask; relu_bits = the sign bits linear_fwd stored for Xact)"""
    lib = _lib.load()
    _req(dY, "dY", ndim=2); _req(W, "W", ndim=2); _req(dX, "dX", ndim=2)
    M, N = dY.shape
    K = W.size(1)
    if W.size(0) != N or dX.size(0) != M or dX.size(1) != K:
        raise RuntimeError("dlrm_amd: linear_bwd_data shape mismatch")
    if Xact is not None:
        _req(Xact, "Xact", ndim=2)
    elif xact_kind != ACT_NONE:
        # (the sign bits alone are not enough here: only the fast GEMM path reads them, every other path of dlrm_linear_bwd_data masks
        # with the fp32 activation — a caller that kept bits only must take dlrm_gemm_bf16's relu_bits_in, functional.MLPFunction)
        raise RuntimeError("dlrm_amd: linear_bwd_data with an activation derivative needs the fp32 activation Xact "
                           "(got xact_kind=%d, Xact=None%s)" % (xact_kind, ", relu_bits given" if relu_bits is not None else ""))
    with _timed("linear_bwd_data"):
        rc = lib.dlrm_linear_bwd_data(M, N, K, C.c_void_p(dY.data_ptr()), _ld(dY), C.c_void_p(W.data_ptr()), _ld(W),
                                      C.c_void_p(Xact.data_ptr()) if Xact is not None else None,
                                      _ld(Xact) if Xact is not None else 0, int(xact_kind if Xact is not None else ACT_NONE),
                                      C.c_void_p(relu_bits.data_ptr()) if (relu_bits is not None and Xact is not None) else None,
                                      C.c_void_p(dX.data_ptr()), _ld(dX), arith_code(arith), _stream(dX))
    _lib.check(rc, "dlrm_linear_bwd_data")
    return dX


# ---- bf16-storage tower (dlrm_cast_bf16 / dlrm_gemm_bf16, include/dlrm_hip.h) -------------------------------------------------
def round32(n: int) -> int:
    return (n + 31) & ~31


def cast_bf16(src: torch.Tensor, Npad: Optional[int] = None, category: str = "cast_bf16") -> torch.Tensor:
    """[M, N] fp32 -> contiguous [M, Npad] bf16 (round to nearest even; zero columns N..Npad-1)"""
    lib = _lib.load()
    _req(src, "src", ndim=2)
    M, N = src.shape
    Npad = N + (N & 1) if Npad is None else int(Npad)
    dst = torch.empty((M, Npad), dtype=torch.bfloat16, device=src.device)
    with _timed(category):
        rc = lib.dlrm_cast_bf16(M, N, Npad, C.c_void_p(src.data_ptr()), _ld(src), C.c_void_p(dst.data_ptr()), Npad, _stream(dst))
    _lib.check(rc, "dlrm_cast_bf16")
    return dst


def cast_bf16_transposed(src: torch.Tensor, Rpad: Optional[int] = None, category: str = "cast_bf16") -> torch.Tensor:
    """[R, C] fp32 -> contiguous [C, Rpad] bf16 = its transpose (zero columns R..Rpad-1): W^T for the data-gradient GEMM"""
    lib = _lib.load()
    _req(src, "src", ndim=2)
    R, Cc = src.shape
    Rpad = R if Rpad is None else int(Rpad)
    dst = torch.empty((Cc, Rpad), dtype=torch.bfloat16, device=src.device)
    with _timed(category):
        rc = lib.dlrm_cast_bf16_transposed(R, Cc, Rpad, C.c_void_p(src.data_ptr()), _ld(src), C.c_void_p(dst.data_ptr()), Rpad, _stream(dst))
    _lib.check(rc, "dlrm_cast_bf16_transposed")
    return dst


CAST_MULTI_MAX = 16


def cast_bf16_multi(items, category: str = "cast_bf16"):
    """bf16 copies of several fp32 matrices in ONE launch (dlrm_cast_bf16_multi).  items: (src [R, C], Cpad or None, Rpad or None) —
    Cpad: also return the row-major copy [R, Cpad] (zero columns C..); Rpad: also return the transposed copy [C, Rpad] (zero columns R..).
    Returns a list of (copy or None, transposed copy or None)."""
    lib = _lib.load()
    out = []
    for k0 in range(0, len(items), CAST_MULTI_MAX):
        chunk = items[k0:k0 + CAST_MULTI_MAX]
        n = len(chunk)
        srcs, lds, R, Cc, dst, ldd, cpad, dstT, lddT, rpad, res = [], [], [], [], [], [], [], [], [], [], []
        for src, Cpad, Rpad in chunk:
            _req(src, "src", ndim=2)
            r_, c_ = src.shape
            d = torch.empty((r_, int(Cpad)), dtype=torch.bfloat16, device=src.device) if Cpad else None
            dT = torch.empty((c_, int(Rpad)), dtype=torch.bfloat16, device=src.device) if Rpad else None
            srcs.append(src.data_ptr()); lds.append(_ld(src)); R.append(r_); Cc.append(c_)
            dst.append(d.data_ptr() if d is not None else 0); ldd.append(int(Cpad) if Cpad else 0); cpad.append(int(Cpad) if Cpad else 0)
            dstT.append(dT.data_ptr() if dT is not None else 0); lddT.append(int(Rpad) if Rpad else 0); rpad.append(int(Rpad) if Rpad else 0)
            res.append((d, dT))
        ia = lambda v: (C.c_int * n)(*v)            # noqa: E731
        with _timed(category):
            rc = lib.dlrm_cast_bf16_multi(n, _lib.ptr_array(srcs), _lib.i64_array(lds), ia(R), ia(Cc), _lib.ptr_array(dst), _lib.i64_array(ldd), ia(cpad),
                                          _lib.ptr_array(dstT), _lib.i64_array(lddT), ia(rpad), _stream(chunk[0][0]))
        _lib.check(rc, "dlrm_cast_bf16_multi")
        out += res
    return out


def gemm_bf16(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor], act: int, Cf: Optional[torch.Tensor],
              Cb: Optional[torch.Tensor], relu_bits_out: Optional[torch.Tensor] = None, relu_bits_in: Optional[torch.Tensor] = None,
              category: str = "linear_fwd", addend: Optional[torch.Tensor] = None, addend2: Optional[torch.Tensor] = None) -> None:
    """Cf (fp32) and/or Cb (bf16) [M, N] = epilogue(A[M, K] @ B[N, K]^T) with bf16 operands in memory (dlrm_gemm_bf16)."""
    lib = _lib.load()
    for t, name in ((A, "A"), (B, "B")):
        if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"dlrm_amd: gemm_bf16 operand {name} must be a 2-D bf16 GPU tensor with contiguous rows")
    M, K = A.shape
    N = B.size(0)
    if B.size(1) != K:
        raise RuntimeError("dlrm_amd: gemm_bf16 reduction lengths differ")
    if Cf is not None:
        _req(Cf, "C", ndim=2)
    if Cb is not None and (Cb.dtype != torch.bfloat16 or tuple(Cb.shape) != (M, N) or Cb.stride(1) != 1):
        raise RuntimeError("dlrm_amd: gemm_bf16 bf16 output must be [M, N] bf16 with contiguous rows")
    out = Cf if Cf is not None else Cb
    with _timed(category):
        rc = lib.dlrm_gemm_bf16(M, N, K, C.c_void_p(A.data_ptr()), A.stride(0), C.c_void_p(B.data_ptr()), B.stride(0),
                                C.c_void_p(bias.data_ptr()) if bias is not None else None, int(act),
                                C.c_void_p(relu_bits_out.data_ptr()) if relu_bits_out is not None else None,
                                C.c_void_p(relu_bits_in.data_ptr()) if relu_bits_in is not None else None,
                                C.c_void_p(addend.data_ptr()) if addend is not None else None, _ld(addend) if addend is not None else 0,
                                C.c_void_p(addend2.data_ptr()) if addend2 is not None else None, _ld(addend2) if addend2 is not None else 0,
                                C.c_void_p(Cf.data_ptr()) if Cf is not None else None, _ld(Cf) if Cf is not None else 0,
                                C.c_void_p(Cb.data_ptr()) if Cb is not None else None, Cb.stride(0) if Cb is not None else 0, _stream(out))
    _lib.check(rc, "dlrm_gemm_bf16")


# ---- arith "bf16x6" from pre-split operands: an fp32 tensor travels as a contiguous [3, rows, cols] bf16 tensor = its planes h, m, l ----

def _planes(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 3 or t.size(0) != 3 or not t.is_contiguous():
        raise RuntimeError(f"dlrm_amd: {name} must be a contiguous [3, rows, cols] bf16 GPU tensor (the planes of an fp32 matrix)")


def round_x6_k(K: int) -> int:
    """reduction length an operand's planes are padded to: the 16-k tile of the planes kernel"""
    return (K + 15) & ~15


def gemm_bf16x6_ok(M: int, N: int, K: int) -> bool:
    """preconditions of dlrm_gemm_bf16x6 for contiguous planes [3, M, K] x [3, N, K]"""
    return bool(_lib.load().dlrm_gemm_bf16x6_supported(M, N, K, K, K)) and 3 * max(M, N) * K < (1 << 31)


def split_bf16x3(src: torch.Tensor, Npad: Optional[int] = None, category: str = "cast_bf16") -> torch.Tensor:
    """[M, N] fp32 -> [3, M, Npad] bf16: the truncation planes h, m, l with src == h + m + l exactly (zero columns N..Npad-1)"""
    lib = _lib.load()
    _req(src, "src", ndim=2)
    M, N = src.shape
    Npad = (N + 7) & ~7 if Npad is None else int(Npad)
    dst = torch.empty((3, M, Npad), dtype=torch.bfloat16, device=src.device)
    with _timed(category):
        rc = lib.dlrm_split_bf16x3(M, N, Npad, C.c_void_p(src.data_ptr()), _ld(src), C.c_void_p(dst.data_ptr()), Npad, M * Npad, _stream(dst))
    _lib.check(rc, "dlrm_split_bf16x3")
    return dst


def split_bf16x3_transposed(src: torch.Tensor, Rpad: Optional[int] = None, category: str = "cast_bf16") -> torch.Tensor:
    """[R, C] fp32 -> [3, C, Rpad] bf16: the planes of its transpose (zero columns R..Rpad-1)"""
    lib = _lib.load()
    _req(src, "src", ndim=2)
    R, Cc = src.shape
    Rpad = R if Rpad is None else int(Rpad)
    dst = torch.empty((3, Cc, Rpad), dtype=torch.bfloat16, device=src.device)
    with _timed(category):
        rc = lib.dlrm_split_bf16x3_transposed(R, Cc, Rpad, C.c_void_p(src.data_ptr()), _ld(src), C.c_void_p(dst.data_ptr()), Rpad, Cc * Rpad, _stream(dst))
    _lib.check(rc, "dlrm_split_bf16x3_transposed")
    return dst


def gemm_bf16x6(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor], act: int, Cf: Optional[torch.Tensor],
                Cp: Optional[torch.Tensor], relu_bits_out: Optional[torch.Tensor] = None, relu_bits_in: Optional[torch.Tensor] = None,
                category: str = "linear_fwd") -> None:
    """Cf (fp32 [M, N]) and/or Cp (planes [3, M, N]) = epilogue(A @ B^T) for operands given as planes A [3, M, K], B [3, N, K] (dlrm_gemm_bf16x6)."""
    lib = _lib.load()
    _planes(A, "A"); _planes(B, "B")
    _, M, K = A.shape
    N = B.size(1)
    if B.size(2) != K:
        raise RuntimeError("dlrm_amd: gemm_bf16x6 reduction lengths differ")
    if Cf is not None:
        _req(Cf, "C", ndim=2)
    if Cp is not None:
        _planes(Cp, "Cp")
        if tuple(Cp.shape) != (3, M, N):
            raise RuntimeError("dlrm_amd: gemm_bf16x6 planes output must be [3, M, N]")
    out = Cf if Cf is not None else Cp
    with _timed(category):
        rc = lib.dlrm_gemm_bf16x6(M, N, K, C.c_void_p(A.data_ptr()), K, M * K, C.c_void_p(B.data_ptr()), K, N * K,
                                  C.c_void_p(bias.data_ptr()) if bias is not None else None, int(act),
                                  C.c_void_p(relu_bits_out.data_ptr()) if relu_bits_out is not None else None,
                                  C.c_void_p(relu_bits_in.data_ptr()) if relu_bits_in is not None else None,
                                  C.c_void_p(Cf.data_ptr()) if Cf is not None else None, _ld(Cf) if Cf is not None else 0,
                                  C.c_void_p(Cp.data_ptr()) if Cp is not None else None, N if Cp is not None else 0, M * N if Cp is not None else 0,
                                  _stream(out))
    _lib.check(rc, "dlrm_gemm_bf16x6")


def linear_bwd_weight_bf16x6(dZ3: torch.Tensor, X3: torch.Tensor, dW: torch.Tensor, dbias: Optional[torch.Tensor] = None,
                             accumulate: bool = False) -> torch.Tensor:
    """dW [N, K_store] fp32 = dZ^T @ X[:, :K_store], dbias = column sums of dZ, from the planes dZ3 [3, M, N], X3 [3, M, K] (read k-strided).
    X3's columns dW.size(1) .. round8(dW.size(1)) must be zero padding."""
    lib = _lib.load()
    _planes(dZ3, "dZ3"); _planes(X3, "X3")
    _req(dW, "dW", ndim=2)
    _, M, N = dZ3.shape
    Kx = X3.size(2)
    K_store = dW.size(1)
    K = (K_store + 7) & ~7
    if X3.size(1) != M or dW.size(0) != N or Kx < K:
        raise RuntimeError("dlrm_amd: linear_bwd_weight_bf16x6 shape mismatch")
    if dbias is not None:
        _req(dbias, "dbias", ndim=1)
    ws = _scratch("wgrad", lib.dlrm_linear_bwd_weight_bf16_workspace_bytes(M, N, K), dW.device)
    with _timed("linear_bwd_weight"):
        rc = lib.dlrm_linear_bwd_weight_bf16x6(M, N, K, K_store, C.c_void_p(dZ3.data_ptr()), N, M * N, C.c_void_p(X3.data_ptr()), Kx, M * Kx,
                                               C.c_void_p(dW.data_ptr()), _ld(dW), C.c_void_p(dbias.data_ptr()) if dbias is not None else None,
                                               int(bool(accumulate)), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dW))
    _lib.check(rc, "dlrm_linear_bwd_weight_bf16x6")
    return dW


def linear_bwd_weight(dY: torch.Tensor, X: torch.Tensor, dW: torch.Tensor, dbias: Optional[torch.Tensor] = None,
                      accumulate: bool = False, use_workspace: bool = True, arith=_lib.ARITH_F32) -> torch.Tensor:
    """dW = dY^T @ X and (optionally) dbias = column sums of dY, one GEMM (+ the split-K slab reduction).
    dW may be NARROWER than X (dW [N, K_store], X [M, K >= K_store]): the extra columns of X are alignment padding
    (zeros) and their gradient is dropped.  use_workspace=False exercises the atomic-accumulation variant."""
    lib = _lib.load()
    _req(dY, "dY", ndim=2); _req(X, "X", ndim=2); _req(dW, "dW", ndim=2)
    M, N = dY.shape
    K = X.size(1)
    K_store = dW.size(1)
    if X.size(0) != M or dW.size(0) != N or K_store > K:
        raise RuntimeError("dlrm_amd: linear_bwd_weight shape mismatch")
    if dbias is not None:
        _req(dbias, "dbias", ndim=1)
        if dbias.numel() != N:
            raise RuntimeError("dlrm_amd: linear_bwd_weight dbias size mismatch")
    ws = _scratch("wgrad", lib.dlrm_linear_bwd_weight_workspace_bytes(M, N, K), dY.device) if use_workspace else None
    with _timed("linear_bwd_weight"):
        common = (C.c_void_p(dY.data_ptr()), _ld(dY), C.c_void_p(X.data_ptr()), _ld(X),
                  C.c_void_p(dW.data_ptr()), _ld(dW),
                  C.c_void_p(dbias.data_ptr()) if dbias is not None else None,
                  int(bool(accumulate)),
                  C.c_void_p(ws.data_ptr()) if ws is not None else None,
                  ws.numel() if ws is not None else 0, arith_code(arith), _stream(dW))
        if K_store == K:
            rc = lib.dlrm_linear_bwd_weight(M, N, K, *common)
        else:
            rc = lib.dlrm_linear_bwd_weight_padded(M, N, K, K_store, *common)
    _lib.check(rc, "dlrm_linear_bwd_weight")
    return dW


# ---- route queries: which kernel a dlrm_linear_* call would launch (include/dlrm_hip.h DLRM_ROUTE_*; host code only, no GPU needed) ----
PATH_FALLBACK, PATH_GEMM3, PATH_GEMV, PATH_SMALLK = 0, 1, 2, 3


class GemmRoute(NamedTuple):
    """the dispatch decision of csrc/gemm.hip, field for field the int[DLRM_ROUTE_FIELDS] of include/dlrm_hip.h"""
    path: int
    tm: int
    tn: int
    frag: int
    epi: int
    nst: int
    arith: int
    sched: int
    splits: int
    kchunk: int
    bits: int
    workspace: int
    atomic: int


def _addr(p) -> Optional[C.c_void_p]:
    """an operand of a route query: a tensor (its data pointer), a plain address, or None — only NULL-ness and alignment are looked at"""
    if p is None:
        return None
    return C.c_void_p(p.data_ptr() if isinstance(p, torch.Tensor) else int(p))


def _route(name: str, *args) -> GemmRoute:
    out = (C.c_int * len(GemmRoute._fields))()
    _lib.check(getattr(_lib.load(), name)(*args, None, out), name)
    return GemmRoute(*out)


def linear_fwd_route(M: int, N: int, K: int, X, ldx: int, W, ldw: int, bias, act: int, Y, ldy: int, relu_bits=None,
                     arith=_lib.ARITH_F32) -> GemmRoute:
    """the route of linear_fwd on these operands (tensors or raw addresses; nothing is read, nothing launched)"""
    return _route("dlrm_linear_fwd_route", M, N, K, _addr(X), ldx, _addr(W), ldw, _addr(bias), int(act), _addr(Y), ldy, _addr(relu_bits),
                  arith_code(arith))


def linear_bwd_data_route(M: int, N: int, K: int, dY, lddy: int, W, ldw: int, Xact, ldxa: int, xact_kind: int, relu_bits, dX, lddx: int,
                          arith=_lib.ARITH_F32) -> GemmRoute:
    """the route of linear_bwd_data (Xact None -> no mask, as in the call)"""
    return _route("dlrm_linear_bwd_data_route", M, N, K, _addr(dY), lddy, _addr(W), ldw, _addr(Xact), ldxa if Xact is not None else 0,
                  int(xact_kind if Xact is not None else ACT_NONE), _addr(relu_bits) if Xact is not None else None, _addr(dX), lddx,
                  arith_code(arith))


def linear_bwd_weight_route(M: int, N: int, K: int, K_store: int, dY, lddy: int, X, ldx: int, dW, lddw: int, dbias=None,
                            accumulate: bool = False, workspace=None, workspace_bytes: int = 0, arith=_lib.ARITH_F32) -> GemmRoute:
    """the route of linear_bwd_weight (K_store < K: the padded form); workspace None = the atomic-accumulation variant"""
    return _route("dlrm_linear_bwd_weight_route", M, N, K, K_store, _addr(dY), lddy, _addr(X), ldx, _addr(dW), lddw, _addr(dbias),
                  int(bool(accumulate)), _addr(workspace), int(workspace_bytes), arith_code(arith))


def linear_head_bwd(dY: torch.Tensor, Y: Optional[torch.Tensor], act: int, X: torch.Tensor, W: torch.Tensor, xact_kind: int,
                    dX: Optional[torch.Tensor], dW: torch.Tensor, dbias: Optional[torch.Tensor], accumulate: bool = False) -> bool:
    """The whole backward of an N == 1 layer in one pass over X (dlrm_linear_head_bwd): dz = dY * act'(Y), dW [1, K] = dz^T X, dbias [1] = sum dz,
    dX [M, K] = (dz W) * xact'(X) — the bits of act_bwd + linear_bwd_weight + linear_bwd_data.  False: the shape is outside the fast path and
    NOTHING was launched (the caller makes the three calls)."""
    lib = _lib.load()
    _req(dY, "dY", ndim=2); _req(X, "X", ndim=2); _req(W, "W", ndim=2); _req(dW, "dW", ndim=2)
    M, K = X.shape
    if dY.size(0) != M or dY.size(1) != 1 or W.shape != (1, K) or dW.shape != (1, K) or (dX is not None and dX.shape != (M, K)):
        raise RuntimeError("dlrm_amd: linear_head_bwd shape mismatch")
    if Y is not None:
        _req(Y, "Y", ndim=2)
    if dX is not None:
        _req(dX, "dX", ndim=2)
    ws = _scratch("wgrad", lib.dlrm_linear_bwd_weight_workspace_bytes(M, 1, K), dY.device)
    if ws is None:
        return False
    with _timed("linear_bwd_weight"):
        rc = lib.dlrm_linear_head_bwd(M, K, C.c_void_p(dY.data_ptr()), _ld(dY), C.c_void_p(Y.data_ptr()) if Y is not None else None,
                                      _ld(Y) if Y is not None else 1, int(act), C.c_void_p(X.data_ptr()), _ld(X), C.c_void_p(W.data_ptr()),
                                      int(xact_kind), C.c_void_p(dX.data_ptr()) if dX is not None else None, _ld(dX) if dX is not None else K,
                                      C.c_void_p(dW.data_ptr()), C.c_void_p(dbias.data_ptr()) if dbias is not None else None,
                                      int(bool(accumulate)), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dW))
    if rc == -4:                                     # DLRM_E_MODE: outside the fast path, nothing launched
        return False
    _lib.check(rc, "dlrm_linear_head_bwd")
    return True


def linear_bwd_weight_bf16_shapes_ok(M: int, N: int, K: int) -> bool:
    """the shapes dlrm_linear_bwd_weight_bf16 takes (csrc/gemm_bf16.hip, weight-gradient form): dW [N, K] from M rows.  The one statement of
    them: the tensor-level check below, MLPFunction's plan and LowRankCrossNetFunction all ask here."""
    return M >= 256 and M % 64 == 0 and N % 8 == 0 and N >= 64 and K >= 64 and BF16_PHASED


def linear_bwd_weight_bf16_ok(M: int, N: int, K: int, dZ16: torch.Tensor, X16: torch.Tensor) -> bool:
    """preconditions of dlrm_linear_bwd_weight_bf16: its shapes (K, the stored width of dW, rounded up to the product's 8), and operands
    that are wide enough, 16-byte aligned and of a pitch that keeps every row so"""
    K = (K + 7) & ~7
    return (linear_bwd_weight_bf16_shapes_ok(M, N, K) and X16.size(1) >= K and dZ16.stride(0) % 8 == 0 and X16.stride(0) % 8 == 0
            and dZ16.data_ptr() % 16 == 0 and X16.data_ptr() % 16 == 0)


def linear_bwd_weight_bf16(dZ16: torch.Tensor, X16: torch.Tensor, dW: torch.Tensor, dbias: Optional[torch.Tensor] = None,
                           accumulate: bool = False) -> torch.Tensor:
    """dW [N, K] fp32 = dZ16[M, N]^T @ X16[M, :K] and dbias = column sums of dZ16, both operands bf16 AS STORED (read k-strided through
    ds_read_b64_tr_b16).  dW may be narrower than the product: X16's columns dW.size(1) .. round8(dW.size(1)) must then be ZERO padding."""
    lib = _lib.load()
    for t, name in ((dZ16, "dZ16"), (X16, "X16")):
        if t.dtype != torch.bfloat16 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"dlrm_amd: linear_bwd_weight_bf16 operand {name} must be a 2-D bf16 GPU tensor with contiguous rows")
    _req(dW, "dW", ndim=2)
    M, N = dZ16.shape
    K_store = dW.size(1)
    K = (K_store + 7) & ~7                       # the product's width; columns K_store.. of X16 are zero padding
    if X16.size(0) != M or dW.size(0) != N or X16.size(1) < K:
        raise RuntimeError("dlrm_amd: linear_bwd_weight_bf16 shape mismatch")
    if dbias is not None:
        _req(dbias, "dbias", ndim=1)
    ws = _scratch("wgrad", lib.dlrm_linear_bwd_weight_bf16_workspace_bytes(M, N, K), dW.device)
    with _timed("linear_bwd_weight"):
        rc = lib.dlrm_linear_bwd_weight_bf16(M, N, K, K_store, C.c_void_p(dZ16.data_ptr()), dZ16.stride(0), C.c_void_p(X16.data_ptr()), X16.stride(0),
                                             C.c_void_p(dW.data_ptr()), _ld(dW), C.c_void_p(dbias.data_ptr()) if dbias is not None else None,
                                             int(bool(accumulate)), C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dW))
    _lib.check(rc, "dlrm_linear_bwd_weight_bf16")
    return dW


def pad_cols(src: torch.Tensor, Kp: int) -> torch.Tensor:
    """[M, K] -> new contiguous [M, Kp] with zero columns K..Kp-1 (one kernel; replaces torch.zeros + slice copy_)."""
    lib = _lib.load()
    _req(src, "src", ndim=2)
    M, K = src.shape
    if Kp < K:
        raise RuntimeError("dlrm_amd: pad_cols target width is smaller than the source")
    dst = torch.empty((M, Kp), dtype=torch.float32, device=src.device)
    if M == 0:
        return dst
    rc = lib.dlrm_pad_cols(M, K, Kp, C.c_void_p(src.data_ptr()), _ld(src), C.c_void_p(dst.data_ptr()), Kp, _stream())
    _lib.check(rc, "dlrm_pad_cols")
    return dst


# ------------------------------------------------------------------------------------------------
# small-batch towers (csrc/tower.hip): all layers of an MLP in one launch per direction
# ------------------------------------------------------------------------------------------------
TOWER_MAX_LAYERS, TOWER_MAX_WIDTH = 8, 512          # DLRM_TOWER_MAX_LAYERS / DLRM_TOWER_MAX_WIDTH of include/dlrm_hip.h


def _int_array(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def tower_ok(M: int, widths: Sequence[int]) -> bool:
    return 0 < M and 1 <= len(widths) - 1 <= TOWER_MAX_LAYERS and all(0 < w <= TOWER_MAX_WIDTH for w in widths)


def tower_fwd(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[Optional[torch.Tensor]], acts: Sequence[int],
              outs: Sequence[torch.Tensor]) -> None:
    """outs[l] = act_l(in_l @ weights[l]^T + biases[l]) for the whole tower, in_0 = x, in_l = outs[l-1]: ONE launch (dlrm_tower_fwd).
    weights[l] is [N_l, K_l] with K_0 == x.size(1) and K_l == N_{l-1}; every outs[l] [M, N_l] is written (backward reads them)."""
    lib = _lib.load()
    L = len(weights)
    _req(x, "x", ndim=2)
    M = x.size(0)
    widths = [x.size(1)] + [w.size(0) for w in weights]
    for l, (w, o) in enumerate(zip(weights, outs)):
        _req(w, "W", ndim=2); _req(o, "out", ndim=2)
        if w.size(1) != widths[l] or o.size(0) != M or o.size(1) != widths[l + 1] or (biases[l] is not None and biases[l].numel() != widths[l + 1]):
            raise RuntimeError("dlrm_amd: tower_fwd shape mismatch at layer %d" % l)
    if len(outs) != L or len(biases) != L or len(acts) != L or not tower_ok(M, widths):
        raise RuntimeError("dlrm_amd: tower_fwd: %d layers of widths %s are outside the small-batch tower kernels" % (L, widths))
    with _timed("linear_fwd"):
        rc = lib.dlrm_tower_fwd(M, L, _int_array(widths), _int_array(acts), C.c_void_p(x.data_ptr()), _ld(x),
                                _lib.ptr_array([w.data_ptr() for w in weights]), _lib.i64_array([_ld(w) for w in weights]),
                                _lib.ptr_array([b.data_ptr() if b is not None else 0 for b in biases]),
                                _lib.ptr_array([o.data_ptr() for o in outs]), _lib.i64_array([_ld(o) for o in outs]), _stream(x))
    _lib.check(rc, "dlrm_tower_fwd")


def tower_bwd(dY: torch.Tensor, weights: Sequence[torch.Tensor], acts: Sequence[int], outs: Sequence[torch.Tensor],
              dZs: Sequence[torch.Tensor], dX: Optional[torch.Tensor], last_act_applied: bool = False) -> None:
    """The data-gradient chain of the tower in ONE launch (dlrm_tower_bwd): dZs[l] [M, N_l] = dL/dz_l of every layer (the operands of
    tower_wgrad) and, when dX is given, the gradient of the tower's input [M, K_0]."""
    lib = _lib.load()
    L = len(weights)
    _req(dY, "dY", ndim=2)
    M = dY.size(0)
    widths = [weights[0].size(1)] + [w.size(0) for w in weights]
    if len(outs) != L or len(dZs) != L or len(acts) != L or dY.size(1) != widths[L] or not tower_ok(M, widths):
        raise RuntimeError("dlrm_amd: tower_bwd argument mismatch")
    for l in range(L):
        _req(outs[l], "out", ndim=2); _req(dZs[l], "dZ", ndim=2)
        if outs[l].shape != (M, widths[l + 1]) or dZs[l].shape != (M, widths[l + 1]) or weights[l].size(1) != widths[l]:
            raise RuntimeError("dlrm_amd: tower_bwd shape mismatch at layer %d" % l)
    if dX is not None:
        _req(dX, "dX", ndim=2)
        if dX.shape != (M, widths[0]):
            raise RuntimeError("dlrm_amd: tower_bwd dX shape mismatch")
    with _timed("linear_bwd_data"):
        rc = lib.dlrm_tower_bwd(M, L, _int_array(widths), _int_array(acts), C.c_void_p(dY.data_ptr()), _ld(dY), int(bool(last_act_applied)),
                                _lib.ptr_array([w.data_ptr() for w in weights]), _lib.i64_array([_ld(w) for w in weights]),
                                _lib.ptr_array([o.data_ptr() for o in outs]), _lib.i64_array([_ld(o) for o in outs]),
                                _lib.ptr_array([z.data_ptr() for z in dZs]), _lib.i64_array([_ld(z) for z in dZs]),
                                C.c_void_p(dX.data_ptr()) if dX is not None else None, _ld(dX) if dX is not None else 0, _stream(dY))
    _lib.check(rc, "dlrm_tower_bwd")


def tower_wgrad(dZs: Sequence[torch.Tensor], ins: Sequence[torch.Tensor], dWs: Sequence[torch.Tensor],
                dbs: Sequence[Optional[torch.Tensor]]) -> None:
    """dWs[l] [N_l, K_store_l] = dZs[l]^T @ ins[l] (K_store_l = dWs[l].size(1) <= ins[l].size(1): trailing padding columns of the input
    are dropped) and dbs[l] = column sums of dZs[l], for ALL layers in one launch, deterministic (dlrm_tower_wgrad)."""
    lib = _lib.load()
    L = len(dZs)
    M = dZs[0].size(0)
    widths = [ins[0].size(1)] + [z.size(1) for z in dZs]
    for l in range(L):
        _req(dZs[l], "dZ", ndim=2); _req(ins[l], "in", ndim=2); _req(dWs[l], "dW", ndim=2)
        if (ins[l].size(0) != M or dZs[l].size(0) != M or ins[l].size(1) != widths[l] or dWs[l].size(0) != widths[l + 1]
                or dWs[l].size(1) > widths[l] or (dbs[l] is not None and (dbs[l].numel() != widths[l + 1] or not dbs[l].is_contiguous()))):
            raise RuntimeError("dlrm_amd: tower_wgrad shape mismatch at layer %d" % l)
    if len(ins) != L or len(dWs) != L or len(dbs) != L or not tower_ok(M, widths):
        raise RuntimeError("dlrm_amd: tower_wgrad argument mismatch")
    wa = _int_array(widths)
    ws = _scratch("tower", int(lib.dlrm_tower_wgrad_workspace_bytes(M, L, wa)), dZs[0].device)
    with _timed("linear_bwd_weight"):
        rc = lib.dlrm_tower_wgrad(M, L, wa, _int_array([w.size(1) for w in dWs]),
                                  _lib.ptr_array([z.data_ptr() for z in dZs]), _lib.i64_array([_ld(z) for z in dZs]),
                                  _lib.ptr_array([i.data_ptr() for i in ins]), _lib.i64_array([_ld(i) for i in ins]),
                                  _lib.ptr_array([w.data_ptr() for w in dWs]), _lib.i64_array([_ld(w) for w in dWs]),
                                  _lib.ptr_array([b.data_ptr() if b is not None else 0 for b in dbs]),
                                  C.c_void_p(ws.data_ptr()), ws.numel(), _stream(dZs[0]))
    _lib.check(rc, "dlrm_tower_wgrad")


def act_bwd(dY: torch.Tensor, Y: torch.Tensor, act: int, dZ: torch.Tensor, dbias: Optional[torch.Tensor]) -> torch.Tensor:
    lib = _lib.load()
    _req(dY, "dY", ndim=2); _req(Y, "Y", ndim=2); _req(dZ, "dZ", ndim=2)
    M, N = dY.shape
    with _timed("act_bwd"):
        rc = lib.dlrm_act_bwd(M, N, C.c_void_p(dY.data_ptr()), _ld(dY), C.c_void_p(Y.data_ptr()), _ld(Y), int(act),
                              C.c_void_p(dZ.data_ptr()), _ld(dZ),
                              C.c_void_p(dbias.data_ptr()) if dbias is not None else None, _stream())
    _lib.check(rc, "dlrm_act_bwd")
    return dZ


# ------------------------------------------------------------------------------------------------
# loss, dense SGD
# ------------------------------------------------------------------------------------------------
def _loss_ws(B: int, device) -> torch.Tensor:
    n = _lib.load().dlrm_loss_workspace_bytes(B)
    return torch.empty(max(int(n) // 4, 1), dtype=torch.float32, device=device)


def bce_loss(p: torch.Tensor, target: torch.Tensor, weights: Optional[torch.Tensor], grad_scale: float,
             want_grad: bool, class_weights=(1.0, 1.0)):
    """returns (loss[1], dp or None); p/target are [B] or [B,1] contiguous.  class_weights = (w_neg, w_pos): the wbce
    weights `loss_ws[T.long()]` of the reference applied inside the kernel."""
    lib = _lib.load()
    _req(p, "p"); _req(target, "target")
    if not p.is_contiguous() or not target.is_contiguous() or p.numel() != target.numel():
        raise RuntimeError("dlrm_amd: bce_loss needs contiguous p/target of equal size")
    B = p.numel()
    loss = torch.empty(1, dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_grad else None
    ws = _loss_ws(B, p.device)
    if weights is not None:
        _req(weights, "weights")
        weights = weights.contiguous()
    with _timed("bce_loss"):
        rc = lib.dlrm_bce_loss(B, C.c_void_p(p.data_ptr()), C.c_void_p(target.data_ptr()),
                               C.c_void_p(weights.data_ptr()) if weights is not None else None,
                               float(class_weights[0]), float(class_weights[1]), float(grad_scale),
                               C.c_void_p(loss.data_ptr()), C.c_void_p(dp.data_ptr()) if dp is not None else None,
                               C.c_void_p(ws.data_ptr()), _stream())
    _lib.check(rc, "dlrm_bce_loss")
    return loss, dp


def bce_logits_loss(z: torch.Tensor, target: torch.Tensor, grad_scale: float, want_grad: bool):
    """BCEWithLogitsLoss(mean) on raw logits (torchrec DLRMTrain): returns (loss[1], dz or None)."""
    lib = _lib.load()
    _req(z, "logits"); _req(target, "target")
    if not z.is_contiguous() or not target.is_contiguous() or z.numel() != target.numel():
        raise RuntimeError("dlrm_amd: bce_logits_loss needs contiguous logits/target of equal size")
    B = z.numel()
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if want_grad else None
    ws = _loss_ws(B, z.device)
    rc = lib.dlrm_bce_logits_loss(B, C.c_void_p(z.data_ptr()), C.c_void_p(target.data_ptr()), float(grad_scale),
                                  C.c_void_p(loss.data_ptr()), C.c_void_p(dz.data_ptr()) if dz is not None else None,
                                  C.c_void_p(ws.data_ptr()), _stream(z))
    _lib.check(rc, "dlrm_bce_logits_loss")
    return loss, dz


def mse_loss(p: torch.Tensor, target: torch.Tensor, grad_scale: float, want_grad: bool):
    lib = _lib.load()
    _req(p, "p"); _req(target, "target")
    if not p.is_contiguous() or not target.is_contiguous() or p.numel() != target.numel():
        raise RuntimeError("dlrm_amd: mse_loss needs contiguous p/target of equal size")
    B = p.numel()
    loss = torch.empty(1, dtype=torch.float32, device=p.device)
    dp = torch.empty_like(p) if want_grad else None
    ws = _loss_ws(B, p.device)
    rc = lib.dlrm_mse_loss(B, C.c_void_p(p.data_ptr()), C.c_void_p(target.data_ptr()), float(grad_scale),
                           C.c_void_p(loss.data_ptr()), C.c_void_p(dp.data_ptr()) if dp is not None else None,
                           C.c_void_p(ws.data_ptr()), _stream())
    _lib.check(rc, "dlrm_mse_loss")
    return loss, dp


def scale_by_scalar(x: torch.Tensor, scalar: torch.Tensor) -> torch.Tensor:
    """x * scalar with `scalar` a 1-element GPU tensor (read on the device)."""
    lib = _lib.load()
    _req(x, "x"); _req(scalar, "scalar")
    if not x.is_contiguous() or scalar.numel() != 1:
        raise RuntimeError("dlrm_amd: scale_by_scalar needs a contiguous tensor and a 1-element scalar")
    y = torch.empty_like(x)
    rc = lib.dlrm_scale_by_device_scalar(x.numel(), C.c_void_p(x.data_ptr()), C.c_void_p(scalar.data_ptr()),
                                         C.c_void_p(y.data_ptr()), _stream())
    _lib.check(rc, "dlrm_scale_by_device_scalar")
    return y


def sgd_dense(w: torch.Tensor, g: torch.Tensor, lr: LrLike) -> None:
    lib = _lib.load()
    _req(w, "w"); _req(g, "g")
    if not w.is_contiguous() or not g.is_contiguous() or w.numel() != g.numel():
        raise RuntimeError("dlrm_amd: sgd_dense needs contiguous tensors of equal size")
    with _timed("sgd_dense"):
        rc = lib.dlrm_sgd_dense(w.numel(), C.c_void_p(w.data_ptr()), C.c_void_p(g.data_ptr()), *_lr_args(lr), _stream())
    _lib.check(rc, "dlrm_sgd_dense")


def sgd_dense_multi(ws: Sequence[torch.Tensor], gs: Sequence[torch.Tensor], lr: LrLike) -> None:
    """w -= lr * g for a whole list of dense parameters, one kernel launch."""
    if not ws:
        return
    lib = _lib.load()
    for w, g in zip(ws, gs):
        _req(w, "w"); _req(g, "g")
        if not w.is_contiguous() or not g.is_contiguous() or w.numel() != g.numel():
            raise RuntimeError("dlrm_amd: sgd_dense_multi needs contiguous tensors of equal size")
    with _timed("sgd_dense"):
        rc = lib.dlrm_sgd_dense_multi(len(ws), _lib.ptr_array([w.data_ptr() for w in ws]),
                                      _lib.ptr_array([g.data_ptr() for g in gs]), _lib.i64_array([w.numel() for w in ws]),
                                      *_lr_args(lr), _stream())
    _lib.check(rc, "dlrm_sgd_dense_multi")


def adagrad_dense(w: torch.Tensor, state_sum: torch.Tensor, g: torch.Tensor, lr: LrLike, eps: float) -> None:
    """state_sum += g*g; w -= lr * g / (sqrt(state_sum) + eps)   (optim/rwsadagrad.py:145-148)"""
    lib = _lib.load()
    _req(w, "w"); _req(g, "g"); _req(state_sum, "state_sum")
    if not (w.is_contiguous() and g.is_contiguous() and state_sum.is_contiguous()) or \
            w.numel() != g.numel() or w.numel() != state_sum.numel():
        raise RuntimeError("dlrm_amd: adagrad_dense needs contiguous tensors of equal size")
    rc = lib.dlrm_adagrad_dense(w.numel(), C.c_void_p(w.data_ptr()), C.c_void_p(state_sum.data_ptr()),
                                C.c_void_p(g.data_ptr()), *_lr_args(lr), float(eps), _stream())
    _lib.check(rc, "dlrm_adagrad_dense")


def set_f32(dsts: Sequence[torch.Tensor], values: Sequence[float]) -> None:
    """dsts[i][0] = values[i] on the current stream, the values travelling in the kernarg (dlrm_set_f32: at most 16 per call)"""
    if len(dsts) != len(values):
        raise RuntimeError("dlrm_amd: set_f32 needs one value per destination")
    for i in range(0, len(dsts), 16):
        d, v = dsts[i:i + 16], values[i:i + 16]
        for t in d:
            _req(t, "scalar")
        rc = _lib.load().dlrm_set_f32(len(d), _lib.ptr_array([t.data_ptr() for t in d]), (C.c_float * len(d))(*[float(x) for x in v]), _stream(d[0]))
        _lib.check(rc, "dlrm_set_f32")


_METRIC_NAMES = ("n", "positives", "tp", "fp", "fn", "tn", "roc_auc", "ap", "round_matches")


def binary_metrics_raw(scores: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Device float64[9] = (n, positives, TP, FP, FN, TN, roc_auc, average_precision, #{rint(score) == target});
    no host synchronisation.  Replaces the numpy / scikit-learn metrics of inference() (dlrm_s_pytorch.py:819-847)."""
    lib = _lib.load()
    _req(scores, "scores"); _req(targets, "targets")
    scores, targets = scores.reshape(-1), targets.reshape(-1)
    if not scores.is_contiguous() or not targets.is_contiguous() or scores.numel() != targets.numel() or scores.numel() == 0:
        raise RuntimeError("dlrm_amd: binary_metrics needs non-empty contiguous scores/targets of equal size")
    n = scores.numel()
    need = lib.dlrm_binary_metrics_workspace_bytes(n)
    if need < 0:
        raise RuntimeError("dlrm_amd: dlrm_binary_metrics_workspace_bytes failed")
    ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=scores.device)
    out = torch.empty(9, dtype=torch.float64, device=scores.device)
    rc = lib.dlrm_binary_metrics(n, C.c_void_p(scores.data_ptr()), C.c_void_p(targets.data_ptr()),
                                 C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, "dlrm_binary_metrics")
    return out


def binary_metrics(scores: torch.Tensor, targets: torch.Tensor) -> dict:
    """The validation_results dictionary of the reference's inference() (recall, precision, f1, ap, roc_auc,
    accuracy; dlrm_s_pytorch.py:828-847) plus `round_accuracy` = its non-mlperf accuracy (:819-821).  One D2H copy."""
    v = dict(zip(_METRIC_NAMES, binary_metrics_raw(scores, targets).tolist()))
    tp, fp, fn, tn, n = v["tp"], v["fp"], v["fn"], v["tn"], v["n"]
    # sklearn's zero_division="warn" convention: an undefined ratio counts as 0
    recall = tp / (tp + fn) if tp + fn > 0 else 0.0
    precision = tp / (tp + fp) if tp + fp > 0 else 0.0
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else 0.0
    v.update(recall=recall, precision=precision, f1=f1, accuracy=(tp + tn) / n, round_accuracy=v["round_matches"] / n)
    return v


def copy_blocks(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor]) -> None:
    """dsts[k][:, :] = srcs[k][:, :] for [M, w_k] row-major views with arbitrary row strides, one launch: torch.cat / split
    along dim 1 without ATen (the "cat" interaction and its backward)."""
    lib = _lib.load()
    if len(srcs) != len(dsts) or not srcs:
        raise RuntimeError("dlrm_amd: copy_blocks needs equally many sources and destinations")
    M = srcs[0].size(0)
    for a_, b_ in zip(srcs, dsts):
        _req(a_, "src", ndim=2); _req(b_, "dst", ndim=2)
        if a_.shape != b_.shape or a_.size(0) != M:
            raise RuntimeError("dlrm_amd: copy_blocks shape mismatch")
    if M == 0:
        return
    widths = (C.c_int * len(srcs))(*[int(a_.size(1)) for a_ in srcs])
    rc = lib.dlrm_copy_blocks(M, len(srcs), _lib.ptr_array([a_.data_ptr() for a_ in srcs]), _lib.i64_array([_ld(a_) for a_ in srcs]),
                              _lib.ptr_array([b_.data_ptr() for b_ in dsts]), _lib.i64_array([_ld(b_) for b_ in dsts]),
                              widths, _stream())
    _lib.check(rc, "dlrm_copy_blocks")


def copy_id_blocks(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor]) -> None:
    """copy_blocks for integer id tensors (int32 / int64, 2-D [M, w_k] views whose rows are contiguous): the id re-layouts of the
    sharded input distribution (ext_dist.kjt_input_dist: destination-major send buffer, source-major -> global-batch-order unpack)
    as ONE strided block-copy launch instead of torch.cat / reshape copies.  Ids travel as 32-bit words."""
    def words(t):
        if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
            raise RuntimeError("dlrm_amd: copy_id_blocks needs 2-D int32 / int64 tensors with contiguous rows")
        return (t.view(torch.int32) if t.dtype == torch.int64 else t).view(torch.float32)
    pairs = [(words(a_), words(b_)) for a_, b_ in zip(srcs, dsts) if a_.numel()]
    if pairs:
        copy_blocks([a_ for a_, _ in pairs], [b_ for _, b_ in pairs])


def bce_elementwise(p: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _req(p, "p"); _req(target, "target")
    if not p.is_contiguous() or not target.is_contiguous() or p.numel() != target.numel():
        raise RuntimeError("dlrm_amd: bce_elementwise needs contiguous p/target of equal size")
    loss = torch.empty_like(p)
    rc = lib.dlrm_bce_elementwise(p.numel(), C.c_void_p(p.data_ptr()), C.c_void_p(target.data_ptr()),
                                  C.c_void_p(loss.data_ptr()), _stream())
    _lib.check(rc, "dlrm_bce_elementwise")
    return loss


def bce_elementwise_bwd(p: torch.Tensor, target: torch.Tensor, dloss: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _req(dloss, "dloss")
    dloss = dloss.contiguous()
    dp = torch.empty_like(p)
    rc = lib.dlrm_bce_elementwise_bwd(p.numel(), C.c_void_p(p.data_ptr()), C.c_void_p(target.data_ptr()),
                                      C.c_void_p(dloss.data_ptr()), C.c_void_p(dp.data_ptr()), _stream())
    _lib.check(rc, "dlrm_bce_elementwise_bwd")
    return dp


def _flat3(*ts):
    n = ts[0].numel()
    for t in ts:
        _req(t, "operand")
        if not t.is_contiguous() or t.numel() != n:
            raise RuntimeError("dlrm_amd: elementwise operands must be contiguous and of equal size")
    return n


def cross_fwd(x0: torch.Tensor, u: torch.Tensor, xl: torch.Tensor, want16: bool = False):
    """x0 * u + xl (DCN-v2 cross layer, elementwise half); want16: also its bf16 rounding (returns (out, out16))"""
    n = _flat3(x0, u, xl)
    out = torch.empty_like(x0)
    out16 = torch.empty(x0.shape, dtype=torch.bfloat16, device=x0.device) if want16 else None
    with _timed("cross_ew"):
        rc = _lib.load().dlrm_cross_fwd(n, C.c_void_p(x0.data_ptr()), C.c_void_p(u.data_ptr()), C.c_void_p(xl.data_ptr()),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(out16.data_ptr()) if want16 else None, _stream(out))
    _lib.check(rc, "dlrm_cross_fwd")
    return (out, out16) if want16 else out


def gemm_bf16_cross(v16: torch.Tensor, W16: torch.Tensor, bias: Optional[torch.Tensor], x0: torch.Tensor, xl: torch.Tensor,
                    want16: bool, category: str = "linear_fwd"):
    """DCN-v2 cross layer, second product with the elementwise half in its epilogue (dlrm_gemm_bf16_cross):
    u = v16 . W16^T + bias;  returns (x_next = x0 * u + xl fp32, bf16(x_next) or None, bf16(u)), or None when the bf16-shaped kernel does not take
    the shape (the caller keeps gemm_bf16 + cross_fwd)."""
    lib = _lib.load()
    M, K = v16.shape
    N = W16.size(0)
    if v16.dtype != torch.bfloat16 or W16.dtype != torch.bfloat16 or W16.size(1) != K or x0.shape != (M, N) or xl.shape != (M, N):
        raise RuntimeError("dlrm_amd: gemm_bf16_cross shape / dtype mismatch")
    _req(x0, "x0", ndim=2); _req(xl, "xl", ndim=2)
    out = torch.empty((M, N), dtype=torch.float32, device=x0.device)
    out16 = torch.empty((M, N), dtype=torch.bfloat16, device=x0.device) if want16 else None
    u16 = torch.empty((M, N), dtype=torch.bfloat16, device=x0.device)
    with _timed(category):
        rc = lib.dlrm_gemm_bf16_cross(M, N, K, C.c_void_p(v16.data_ptr()), v16.stride(0), C.c_void_p(W16.data_ptr()), W16.stride(0),
                                      C.c_void_p(bias.data_ptr()) if bias is not None else None,
                                      C.c_void_p(x0.data_ptr()), _ld(x0), C.c_void_p(xl.data_ptr()), _ld(xl),
                                      C.c_void_p(u16.data_ptr()), u16.stride(0), C.c_void_p(out.data_ptr()), _ld(out),
                                      C.c_void_p(out16.data_ptr()) if out16 is not None else None, out16.stride(0) if out16 is not None else 0,
                                      _stream(out))
    if rc == -4:                       # DLRM_E_MODE: outside the bf16-shaped kernel's preconditions
        return None
    _lib.check(rc, "dlrm_gemm_bf16_cross")
    return out, out16, u16


def cross_bwd(g: torch.Tensor, x0: torch.Tensor, u: torch.Tensor, dx0: torch.Tensor, accumulate: bool, out: str = "f32"):
    """du = g * x0 (out "f32": fp32 tensor; "bf16": only its bf16 rounding — what a bf16-storage weight / data gradient reads); dx0 (+)= g * u
    (u: the fp32 tensor, or the bf16 copy gemm_bf16_cross stored)"""
    n = _flat3(g, x0, dx0)
    if u.dtype == torch.bfloat16:
        if not u.is_contiguous() or u.numel() != n:
            raise RuntimeError("dlrm_amd: elementwise operands must be contiguous and of equal size")
    else:
        _flat3(g, u)
    du = torch.empty_like(g) if out == "f32" else None
    du16 = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device) if out == "bf16" else None
    with _timed("cross_ew"):
        rc = _lib.load().dlrm_cross_bwd(n, C.c_void_p(g.data_ptr()), C.c_void_p(x0.data_ptr()),
                                        C.c_void_p(u.data_ptr()) if u.dtype != torch.bfloat16 else None,
                                        C.c_void_p(u.data_ptr()) if u.dtype == torch.bfloat16 else None,
                                        C.c_void_p(du.data_ptr()) if du is not None else None,
                                        C.c_void_p(du16.data_ptr()) if du16 is not None else None,
                                        C.c_void_p(dx0.data_ptr()), int(bool(accumulate)), _stream(g))
    _lib.check(rc, "dlrm_cross_bwd")
    return du if out == "f32" else du16


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    n = _flat3(a, b)
    out = torch.empty_like(a)
    with _timed("cross_ew"):
        rc = _lib.load().dlrm_add(n, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr()), _stream(a))
    _lib.check(rc, "dlrm_add")
    return out


def clamp(x: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    lib = _lib.load()
    _req(x, "x")
    if not x.is_contiguous():
        raise RuntimeError("dlrm_amd: clamp needs a contiguous tensor")
    y = torch.empty_like(x)
    _lib.check(lib.dlrm_clamp(x.numel(), C.c_void_p(x.data_ptr()), float(lo), float(hi), C.c_void_p(y.data_ptr()), _stream()),
               "dlrm_clamp")
    return y


def clamp_bwd(x: torch.Tensor, lo: float, hi: float, dy: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _req(dy, "dy")
    dy = dy.contiguous()
    dx = torch.empty_like(x)
    _lib.check(lib.dlrm_clamp_bwd(x.numel(), C.c_void_p(x.data_ptr()), float(lo), float(hi), C.c_void_p(dy.data_ptr()),
                                  C.c_void_p(dx.data_ptr()), _stream()), "dlrm_clamp_bwd")
    return dx


def device_info(device: int = 0) -> dict:
    lib = _lib.load()
    cu, lds, hbm = C.c_int(), C.c_int(), C.c_int64()
    name = C.create_string_buffer(256)
    rc = lib.dlrm_hip_device_info(device, C.byref(cu), C.byref(lds), C.byref(hbm), name, 256)
    _lib.check(rc, "dlrm_hip_device_info")
    return {"name": name.value.decode(), "cu_count": cu.value, "lds_bytes": lds.value, "hbm_bytes": hbm.value,
            "build": lib.dlrm_hip_build_info().decode(), "abi": lib.dlrm_hip_abi_version()}


# The "one lookup per bag" proof (state and logic) lives in dlrm_amd/iota.py; its public names stay attributes of this module.  Imported
# HERE, at the end: iota uses _timed, _stream and wait_spinning of this module, so it can only be loaded once they exist.
from .iota import (IOTA_STATS, mark_one_lookup_per_bag, offsets_are_iota, offsets_are_iota_finish,  # noqa: E402,F401
                   offsets_are_iota_start, offsets_iota_state)
