"""Capture and replay of a HIP graph, the one protocol of graph.GraphedTrainStep and graph_forward.GraphedForward: static inputs
(_clone_struct, _check_struct, the torch copies of _copy_struct, the C arrays of StagePlan and of RaggedPlan), Capture (warm up on a
private stream, capture relaxed, pin the scratch workspaces, take the raw hipGraphExec_t), InFlight (one replay in flight) and replay (one
C call: csrc/replay.h)."""
from __future__ import annotations

import ctypes as C
import os as _os
from typing import Optional, Sequence, Union

import torch

from . import _lib, ops

TensorOrList = Union[torch.Tensor, Sequence[torch.Tensor]]

STAGE_MEMCPY_MAX = 4        # requests of at most this many segments are staged with one hipMemcpyAsync each (stacked inputs), more with one
                            # dlrm_stage_inputs launch (profiles/graph_forward/rates.md)
STAGE_SEGS_PER_LAUNCH = 64  # DLRM_MAX_STAGE_SEGS of csrc/stage.hip
MEMCPY_ALWAYS = 2 ** 31 - 1  # the threshold of a training step: one hipMemcpyAsync per segment whatever their number (dlrm_graph_replay)


# ------------------------------------------------------------------------------------------------ static inputs
def _clone_struct(x: TensorOrList):
    """Static copies; tensors that appear several times in a list (e.g. one shared offsets tensor for all tables) are
    cloned once and aliased the same way."""
    if isinstance(x, torch.Tensor):
        return x.clone()
    seen = {}
    for t in x:
        if id(t) not in seen:
            seen[id(t)] = t.clone()
    return [seen[id(t)] for t in x]


def _check_struct(dst: TensorOrList, src: TensorOrList) -> None:
    """the refusals of a request that is not of the captured shapes"""
    if isinstance(dst, torch.Tensor):
        if not isinstance(src, torch.Tensor) or src.shape != dst.shape or src.dtype != dst.dtype:
            raise RuntimeError("dlrm_amd.graph: input shape/dtype differs from the captured step")
        return
    if isinstance(src, torch.Tensor) or len(src) != len(dst):
        raise RuntimeError("dlrm_amd.graph: input structure differs from the captured step")
    for d, s_ in zip(dst, src):
        if s_.shape != d.shape or s_.dtype != d.dtype:
            raise RuntimeError("dlrm_amd.graph: input shape/dtype differs from the captured step "
                               "(variable-length multi-hot batches cannot be replayed)")


def _copy_struct(dst: TensorOrList, src: TensorOrList) -> None:
    """static buffers <- the caller's tensors, an ATen copy_ for every distinct tensor whose storage differs, after the checks of
    _check_struct.  (All copies in ONE launch of the library's block copy was measured too: building its views costs the host more than
    the four copy_ calls it replaces, and the host is what the GPU waits for between replays — Criteo-Kaggle graph 0.378 -> 0.406 ms,
    profiles/round5/kaggle_towers.md.)"""
    _check_struct(dst, src)
    if isinstance(dst, torch.Tensor):
        dst, src = [dst], [src]
    done = set()
    for d, s_ in zip(dst, src):
        if id(d) in done or s_.data_ptr() == d.data_ptr():
            continue
        done.add(id(d))
        # one copy per distinct tensor.  (torch._foreach_copy_ on int64 lists raised GPU memory faults on
        # torch 2.10 + ROCm 7 at B = 65536 — profiles/r02/graph_probe.md; pass stacked [T, B] index / offset tensors to
        # make this a single copy.)
        d.copy_(s_, non_blocking=True)


class StagePlan:
    """The segment list of one graph: static buffers <- a request of the same input structure, as the ctypes arrays of dlrm_graph_replay /
    dlrm_forward_replay / dlrm_stage_inputs.  Built ONCE per graph (destinations never change); patch() writes the source pointers and
    lengths of a request.  A segment whose source is its destination (the caller handed the static buffer back) is skipped by the C side.
      a tensor   one segment: a request's n rows are the head of the static [B, m] buffer;
      a list     one segment per DISTINCT static tensor (one shared offsets tensor is staged once), the request's tensor at the first
                 position that maps to it;
      stacked    one segment, the whole [T, n'] tensor — unless its group is named in `by_rows`: then the T rows, each into the head of
                 its row of the static buffer.  A BUCKET names its stacked indices there whatever the width of the request the plan is
                 built from: a later request of the same key may be narrower, and T rows laid end to end are not the heads of T rows.
    A group whose static is None is not staged (a bucket's offsets never change).  patch() refuses a segment longer than its destination."""

    def __init__(self, statics: Sequence, like: Sequence, by_rows: Sequence[int] = ()):
        self.entries = []       # (group, position in the list or None, row or None)
        dst, cap = [], []
        for g, (s, r) in enumerate(zip(statics, like)):
            if s is None:
                continue
            if isinstance(s, torch.Tensor):
                if not isinstance(r, torch.Tensor) or r.dtype != s.dtype or r.dim() != s.dim():
                    raise RuntimeError("dlrm_amd.graph: input structure differs from the captured forward")
                if g in by_rows:
                    if s.dim() != 2 or r.size(0) != s.size(0) or r.size(1) > s.size(1) or (s.size(1) > 1 and s.stride(1) != 1):
                        raise RuntimeError("dlrm_amd.graph: a stacked input does not fit its static buffer")
                    for k in range(s.size(0)):
                        self.entries.append((g, None, k))
                        dst.append(s.data_ptr() + k * s.stride(0) * s.element_size())
                        cap.append(s.size(1) * s.element_size())
                else:
                    if s.dim() == 2 and r.size(1) != s.size(1):
                        raise RuntimeError("dlrm_amd.graph: a stacked input narrower than its static buffer is staged by rows (by_rows)")
                    self.entries.append((g, None, None))
                    dst.append(s.data_ptr())
                    cap.append(s.numel() * s.element_size())
                continue
            if isinstance(r, torch.Tensor) or len(r) != len(s):
                raise RuntimeError("dlrm_amd.graph: input structure differs from the captured forward")
            seen = set()
            for k, t in enumerate(s):
                if id(t) in seen:
                    continue
                seen.add(id(t))
                self.entries.append((g, k, None))
                dst.append(t.data_ptr())
                cap.append(t.numel() * t.element_size())
        self.n = len(dst)
        m = max(self.n, 1)
        self.cap = cap
        self.device = next((t.device for s in statics if s is not None for t in ([s] if isinstance(s, torch.Tensor) else s)), None)
        # flat: every static tensor that a segment fills from end to end is one run of bytes
        self.flat = all((statics[g] if k is None else statics[g][k]).is_contiguous() for g, k, row in self.entries if row is None)
        self.dst = (C.c_void_p * m)(*dst)
        self.src = (C.c_void_p * m)()
        self.nbytes = (C.c_int64 * m)()

    def takes(self, request: Sequence) -> bool:
        """is every tensor patch() would read contiguous and on the static buffers' device?  (Otherwise torch's copy_: _copy_struct.)"""
        dev = self.device               # (not flat: a static buffer kept the strides of a permuted first input, no single run of bytes)
        return self.flat and all(t.device == dev and t.is_contiguous() for t in (request[g] if k is None else request[g][k] for g, k, _ in self.entries))

    def patch(self, request: Sequence) -> None:
        src, nbytes, cap = self.src, self.nbytes, self.cap
        for j, (g, k, row) in enumerate(self.entries):
            t = request[g] if k is None else request[g][k]
            if row is None:
                p, nb = t.data_ptr(), t.numel() * t.element_size()
            else:
                nb = t.size(1) * t.element_size()
                p = t.data_ptr() + row * nb
            if nb > cap[j]:
                raise RuntimeError("dlrm_amd.graph: an input is larger than the static buffer it is staged into")
            src[j], nbytes[j] = p, nb

    def launches(self, memcpy_max: int) -> int:
        """kernel launches of one staging (0: the memcpy path)"""
        return 0 if self.n <= memcpy_max else (self.n + STAGE_SEGS_PER_LAUNCH - 1) // STAGE_SEGS_PER_LAUNCH


class RaggedPlan:
    """The staging of one RAGGED bucket (graph_forward.py), as the ctypes arguments of dlrm_stage_ragged / dlrm_forward_replay_ragged.
    statics = (X [bucket, m], offsets, ids): lists of 1-D tensors (ids k of `caps[k]` elements, offsets of `bucket`; one tensor object
    at several positions is ONE buffer) or stacked [T, Lcap] / [T, bucket] tensors, staged by rows.  Destinations and capacities are
    fixed here; patch() writes the sources, n and nnz_k of a request and keeps shift_k = cap_k - nnz_k (the C side derives the same from
    nnz and cap: ids go to ids_static[shift_k:], offsets become shift_k + clamp(off, 0, nnz_k), tail bags start at cap_k).  An offsets
    buffer shared by several tables needs one capacity (refused here otherwise) and one nnz (refused by patch)."""

    def __init__(self, statics: Sequence, caps: Sequence[int], bucket: int):
        Xs, Os, Is = statics
        self.bucket, self.caps = int(bucket), tuple(int(c) for c in caps)
        self.stacked = isinstance(Is, torch.Tensor)
        T = Is.size(0) if self.stacked else len(Is)
        if isinstance(Os, torch.Tensor) != self.stacked or (Os.size(0) if self.stacked else len(Os)) != T or len(self.caps) != T:
            raise RuntimeError("dlrm_amd.graph: a ragged bucket needs offsets and indices of one structure and one capacity per table")
        if Xs.dim() != 2 or Xs.size(0) != self.bucket or not Xs.is_contiguous() or min(self.caps, default=1) < 1:
            raise RuntimeError("dlrm_amd.graph: a ragged bucket needs a contiguous [bucket, m] dense buffer and capacities >= 1")
        self.T, self.idt = T, Is.dtype if self.stacked else Is[0].dtype
        self.elem = 8 if self.idt == torch.int64 else 4
        self.x_dst, self.x_row = Xs.data_ptr(), Xs.size(1) * Xs.element_size()
        self.x_shape, self.x_dtype = Xs.size(1), Xs.dtype
        # (table whose nnz the segment takes, destination, capacity); off_tabs: every table that shares the offsets buffer
        self.ids_tab, self.off_tab, self.off_tabs = [], [], []
        ids_dst, ids_cap, off_dst, off_cap = [], [], [], []
        if self.stacked:
            if tuple(Is.shape) != (T, self.caps[0]) or tuple(Os.shape) != (T, self.bucket) or len(set(self.caps)) != 1 or Os.dtype != self.idt \
                    or not (Is.is_contiguous() and Os.is_contiguous()):
                raise RuntimeError("dlrm_amd.graph: stacked ragged buffers are [T, Lcap] and [T, bucket] with one capacity for all tables")
            for k in range(T):
                self.ids_tab.append(k)
                ids_dst.append(Is.data_ptr() + k * self.caps[0] * self.elem)
                ids_cap.append(self.caps[0])
                self.off_tab.append(k)
                self.off_tabs.append((k,))
                off_dst.append(Os.data_ptr() + k * self.bucket * self.elem)
                off_cap.append(self.caps[0])
        else:
            seen: dict = {}
            for k, t in enumerate(Is):
                if t.dtype != self.idt or t.numel() != self.caps[k] or not t.is_contiguous():
                    raise RuntimeError("dlrm_amd.graph: the static ids of table %d are not %d contiguous elements of one dtype" % (k, self.caps[k]))
                if id(t) not in seen:
                    seen[id(t)] = k
                    self.ids_tab.append(k)
                    ids_dst.append(t.data_ptr())
                    ids_cap.append(self.caps[k])
            seen = {}
            for k, t in enumerate(Os):
                if t.dtype != self.idt or t.numel() != self.bucket or not t.is_contiguous():
                    raise RuntimeError("dlrm_amd.graph: the static offsets of table %d are not %d contiguous elements of the ids' dtype" % (k, self.bucket))
                j = seen.setdefault(id(t), len(self.off_tab))
                if j == len(self.off_tab):
                    self.off_tab.append(k)
                    self.off_tabs.append(())
                    off_dst.append(t.data_ptr())
                    off_cap.append(self.caps[k])
                elif self.caps[k] != off_cap[j]:
                    raise RuntimeError("dlrm_amd.graph: tables that share one offsets tensor need one lookup capacity")
                self.off_tabs[j] += (k,)
        self.n_ids, self.n_off = len(ids_dst), len(off_dst)
        self.ids_dst = (C.c_void_p * self.n_ids)(*ids_dst)
        self.ids_src = (C.c_void_p * self.n_ids)()
        self.ids_nnz = (C.c_int64 * self.n_ids)()
        self.ids_cap = (C.c_int64 * self.n_ids)(*ids_cap)
        self.off_dst = (C.c_void_p * self.n_off)(*off_dst)
        self.off_src = (C.c_void_p * self.n_off)()
        self.off_nnz = (C.c_int64 * self.n_off)()
        self.off_cap = (C.c_int64 * self.n_off)(*off_cap)
        self.x_src, self.x_bytes, self.rows = 0, 0, 0
        self.nnz = [0] * T              # of the request patched last, per table
        self.shift = list(self.caps)
        self._segs = self.n_off

    def patch(self, request: Sequence) -> None:
        X, lS_o, lS_i = request
        n = X.size(0)
        if X.dim() != 2 or X.size(1) != self.x_shape or X.dtype != self.x_dtype or n > self.bucket or not X.is_contiguous():
            raise RuntimeError("dlrm_amd.graph: the dense input does not fit the ragged bucket (rows, width, dtype, or not contiguous)")
        if isinstance(lS_i, torch.Tensor) != self.stacked or isinstance(lS_o, torch.Tensor) != self.stacked:
            raise RuntimeError("dlrm_amd.graph: input structure differs from the captured forward")
        T, caps, elem = self.T, self.caps, self.elem
        if self.stacked:
            if lS_i.dim() != 2 or lS_o.dim() != 2 or lS_i.size(0) != T or lS_o.size(0) != T or lS_i.dtype != self.idt or lS_o.dtype != self.idt:
                raise RuntimeError("dlrm_amd.graph: input structure differs from the captured forward")
            w = lS_i.size(1)
            if w > caps[0] or lS_o.size(1) != n or not (lS_i.is_contiguous() and lS_o.is_contiguous()):
                raise RuntimeError("dlrm_amd.graph: a ragged request does not fit its bucket (lookups above the capacity, not n offsets, "
                                   "or not contiguous)")
            nnz = [w] * T
            ip, op = lS_i.data_ptr(), lS_o.data_ptr()
            for k in range(T):
                self.ids_src[k], self.ids_nnz[k] = (ip + k * w * elem) if w else None, w
                self.off_src[k], self.off_nnz[k] = (op + k * n * elem) if n else None, w
        else:
            if len(lS_i) != T or len(lS_o) != T:
                raise RuntimeError("dlrm_amd.graph: input structure differs from the captured forward")
            nnz = [t.numel() for t in lS_i]
            for k in range(T):
                if nnz[k] > caps[k] or lS_o[k].numel() != n or lS_i[k].dtype != self.idt or lS_o[k].dtype != self.idt \
                        or not (lS_i[k].is_contiguous() and lS_o[k].is_contiguous()):
                    raise RuntimeError("dlrm_amd.graph: a ragged request does not fit its bucket (lookups above the capacity, not n offsets, "
                                       "another index dtype, or not contiguous)")
            for j, k in enumerate(self.ids_tab):
                self.ids_src[j], self.ids_nnz[j] = (lS_i[k].data_ptr() if nnz[k] else None), nnz[k]
            for j, k in enumerate(self.off_tab):
                if any(nnz[q] != nnz[k] for q in self.off_tabs[j]):
                    raise RuntimeError("dlrm_amd.graph: tables that share one offsets tensor need the same number of lookups")
                self.off_src[j], self.off_nnz[j] = (lS_o[k].data_ptr() if n else None), nnz[k]
        self.x_src, self.x_bytes, self.rows = (X.data_ptr() if n else 0), n * self.x_row, n
        self.nnz = nnz
        self.shift = [c - z for c, z in zip(caps, nnz)]
        self._segs = (1 if n else 0) + sum(1 for j in range(self.n_ids) if self.ids_nnz[j]) + self.n_off

    def launches(self, memcpy_max: int = 0) -> int:
        """stage_ragged_kernel launches of the request patched last (there is no memcpy path: the offsets are computed)"""
        return (self._segs + STAGE_SEGS_PER_LAUNCH - 1) // STAGE_SEGS_PER_LAUNCH

    def args(self) -> tuple:
        return (C.c_void_p(self.x_dst), C.c_void_p(self.x_src), self.x_bytes, self.n_ids, self.ids_dst, self.ids_src, self.ids_nnz,
                self.ids_cap, self.n_off, self.off_dst, self.off_src, self.off_nnz, self.off_cap, self.rows, self.bucket, self.elem)


def stage(plan, request: Sequence, stream) -> None:
    """request -> static buffers on `stream`, outside a replay call: dlrm_stage_inputs, one launch per 64 copying segments
    (a RaggedPlan: dlrm_stage_ragged)"""
    plan.patch(request)
    if isinstance(plan, RaggedPlan):
        _lib.check(_lib.load().dlrm_stage_ragged(*plan.args(), C.c_void_p(stream.cuda_stream)), "dlrm_stage_ragged")
    elif plan.n:
        _lib.check(_lib.load().dlrm_stage_inputs(plan.n, plan.dst, plan.src, plan.nbytes, C.c_void_p(stream.cuda_stream)), "dlrm_stage_inputs")


# ------------------------------------------------------------------------------------------------ capture
class Capture:
    """One captured graph: the private `stream` it is warmed up and captured on (captures may share one), the torch `graph`, its raw
    hipGraphExec_t `exec` (None: torch's own replay), the scratch workspaces it pins and its static output `out`."""
    __slots__ = ("stream", "graph", "exec", "pinned_ws", "out")

    def __init__(self, stream: Optional[torch.cuda.Stream] = None):
        self.stream = stream
        self.graph = self.exec = self.pinned_ws = self.out = None

    def _join(self, dev):
        cur = torch.cuda.current_stream(dev)
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(cur)
        return cur

    def run(self, dev, body):
        """body() on the capture stream, joined both ways — warm-up: attributes, per-stream scratch and pools as the graph will see them"""
        cur = self._join(dev)
        with torch.cuda.stream(self.stream):
            r = body()
        cur.wait_stream(self.stream)
        return r

    def record(self, dev, body, raw: bool = True):
        """Capture body() -> what it returned; it only RECORDS.  Device state written on the current stream before is covered by the join."""
        if ops.timers is not None:
            raise RuntimeError("dlrm_amd.graph: per-kernel event timers cannot be recorded inside a graph capture")
        self.reset()
        cur = self._join(dev)
        graph = torch.cuda.CUDAGraph()
        # "relaxed": a backward runs on the autograd engine's thread, which must be let enqueue into the capturing stream; a forward polls
        # events of finished offsets proofs and reads the pinned error block while the stream captures
        with torch.cuda.graph(graph, stream=self.stream, capture_error_mode="relaxed"):
            r = body()
        self.graph = graph
        # the graph holds raw pointers into the cached scratch workspaces: pin those tensors so that a later, larger
        # request elsewhere (which replaces the cache entry) cannot free memory the replays still use
        self.pinned_ws = [w for (_, d_, _), w in ops._scratch_ws.items() if d_ == dev]
        if raw:
            try:
                self.exec = int(graph.raw_cuda_graph_exec())
            except Exception:                               # noqa: BLE001 - a torch without the raw handle: keep its own replay
                self.exec = None
        cur.wait_stream(self.stream)
        return r

    def reset(self) -> None:
        """forget the graph and with it the raw handle (a dangling one must never reach a replay call); the caller has waited for the replay"""
        if self.graph is not None:
            self.graph.reset()
        self.graph = self.exec = self.pinned_ws = self.out = None


# At most ONE replay in flight, and a full stream synchronisation between replays.  Two launches of the same executable graph queued
# behind each other overlapped on ROCm 7.2 (they share every intermediate buffer), and event waits alone were not enough once the
# application synchronised the stream somewhere in between (profiles/r02/graph_probe.md, b and d): the pattern that was clean in every
# probe is "synchronise the stream after every replay", so that is what happens before the static inputs are touched again — inside the
# replay call (its sync_first argument) or by wait().  At Criteo-Terabyte sizes the GPU is the bottleneck (the wait costs one launch
# latency per step); at launch-bound sizes the replay has finished long before the host gets here.
class InFlight:
    """the rule above: `pending` is set by replay() and cleared by wait(); DLRM_GTS_SERIALIZE=0 turns the rule off (probes only)"""
    def __init__(self):
        self.serialize = _os.environ.get("DLRM_GTS_SERIALIZE", "1") == "1"
        self.pending = False

    def wait(self, stream, always: bool = False) -> None:
        if self.pending or always:
            ops.wait_spinning(stream)       # (polled, not slept on: see ops.wait_spinning)
            self.pending = False


def replay(cap: Capture, flight: InFlight, stream, plan: StagePlan, request: Sequence, memcpy_max: int = MEMCPY_ALWAYS,
           scalars=None, staged: bool = False) -> None:
    """One replay of `cap` on `stream`.  With the raw handle: the plan patched and ONE C call — wait for the replay in flight, stage, write
    `scalars` ((count <= 16, device pointers, values) or None), hipGraphLaunch: dlrm_graph_replay for memcpy_max == MEMCPY_ALWAYS (a
    step), else dlrm_forward_replay (no scalars), dlrm_forward_replay_ragged for a RaggedPlan.  Without it the torch calls: wait, dlrm_stage_inputs, dlrm_set_f32, CUDAGraph.replay().
    staged: the caller has waited and staged already, with torch copies (_copy_struct) — the torch calls without the first two."""
    n, sdst, sval = scalars or (0, None, None)
    lib = _lib.load()
    where = C.c_void_p(stream.cuda_stream)
    if cap.exec is not None and not staged:
        plan.patch(request)
        if isinstance(plan, RaggedPlan):        # (a ragged bucket of GraphedForward: the same protocol, its own staging)
            rc = lib.dlrm_forward_replay_ragged(*plan.args(), C.c_void_p(cap.exec), int(flight.pending), where)
            _lib.check(rc, "dlrm_forward_replay_ragged")
        elif memcpy_max >= MEMCPY_ALWAYS:
            rc = lib.dlrm_graph_replay(plan.n, plan.dst, plan.src, plan.nbytes, n, sdst, sval, C.c_void_p(cap.exec), int(flight.pending), where)
            _lib.check(rc, "dlrm_graph_replay")
        else:
            rc = lib.dlrm_forward_replay(plan.n, plan.dst, plan.src, plan.nbytes, memcpy_max, C.c_void_p(cap.exec), int(flight.pending), where)
            _lib.check(rc, "dlrm_forward_replay")
    else:
        if not staged:
            flight.wait(stream)
            stage(plan, request, stream)
        if n:                        # the new step sizes go in front of the launch on the same stream
            _lib.check(lib.dlrm_set_f32(n, sdst, sval, where), "dlrm_set_f32")
        cap.graph.replay()
    flight.pending = flight.serialize
