"""Whole-forward HIP graph for small-batch serving: `model(X, lS_o, lS_i)` under no_grad captured once per shape and replayed with one
host call per request (dlrm_forward_replay: wait for the previous replay, stage the request into the static buffers, hipGraphLaunch).
The counterpart of graph.GraphedTrainStep, which captures a training step and therefore refuses the inference models (packed tables, int8 /
fp16 towers); both stand on graph_core.py (Capture, InFlight, StagePlan, replay); re-exported as dlrm_amd.graph.GraphedForward.

    fwd = GraphedForward(model, batch_sizes=(64, 256, 2048))
    Z = fwd(X, lS_o, lS_i)          # [n, 1] view of a static buffer, valid until the next call

What is captured is the model's own forward, unchanged: every table kind and tower kind whose forward is built.  The rules of
graph_core.Capture hold (own stream, no event timers, the scratch workspaces of the capture pinned, single stream, single process).

Shapes.  Without `batch_sizes` every distinct request shape gets its own graph (at most `max_exact_shapes`, least recently used dropped).
With `batch_sizes` a request of n rows whose lookup structure is FIXED — table k has exactly P_k lookups in every bag, offsets ==
P_k * arange(n), proven on the caller's tensors — runs in the smallest bucket >= n: its rows go to the head of the bucket's static
buffers (the static offsets are P_k * arange(bucket) and never change), Z[:n] comes back.  Rows n.. keep what earlier requests left there or
the zeros of the capture: every sample's forward is independent, so rows < n do not depend on them — with one exception, the int8 towers,
whose activation range is taken over the whole batch tensor; such a model is refused with buckets.  The answer of a bucket is the eager
forward on the padded batch, bit for bit (the library picks GEMM variants by M: the eager forward at n may sum in another order).  A ragged
request, or n above the largest bucket, takes an exact-shape graph — unless ragged buckets are asked for:

Ragged buckets (`lookup_capacity=c`, an int or one per table; opt-in, needs `batch_sizes`).  A multi-hot request whose bags have their own
lengths — the reference's default data — is a new shape tuple almost every time, and exact-shape graphs then capture per request.  A ragged
bucket holds, per table, static ids of Lcap_k = bucket * c_k lookups and `bucket` static offsets, and is captured ONCE with nnz = Lcap_k.
Every lookup kernel takes nnz by value (bag b is [off[b], off[b+1]), the last one ends at nnz), so padding the ids on the right would hand
the padding to the last bag; a request of nnz_k <= Lcap_k ids is RIGHT-ALIGNED instead, shift_k = Lcap_k - nnz_k:
    ids_static[shift_k:] = ids_req;   off_static[b] = shift_k + clamp(off_req[b], 0, nnz_k) for b < n,   Lcap_k for n <= b < bucket
(one dlrm_stage_ragged launch inside the replay call: csrc/stage.hip, graph_core.RaggedPlan).  Real bags keep their ids in order, the last
real bag ends at off_static[n] = Lcap_k (or at the baked nnz when n == bucket), tail bags are empty and pool to zero, and what lies in front
of off_static[0] — zeros, or an earlier request's valid ids — is never pooled: every forward lookup (dlrm_emb_fwd, _bf16, _quant, _qr, _md)
reads ids one element at a time inside [off[b], off[b+1]) only, so any 4-byte alignment of the shifted ids is fine.  dlrm_pool_weights_gather
(weighted pooling) does walk all Lcap_k ids: harmless, stale ids are valid ids and their weights are read by no bag.  A lane sums a bag's
rows in index order wherever the bag sits, so rows < n are the bits of the eager forward on the padded batch (X padded with zero rows,
offsets cat(off_req, full(bucket - n, nnz_k)), the request's ids).  The clamp changes nothing for well-formed offsets; for any others it keeps
the captured kernels inside the static ids.  Routing: a fixed-length bucket where fixed_bag_lengths succeeds, else a ragged bucket when every
table has n offsets and nnz_k <= Lcap_k (tables that share a tensor object: one nnz, one capacity; stacked inputs: one capacity), else an
exact-shape graph.  The key holds no nnz.  The train step (graph.GraphedTrainStep) has no such form: its backward and sorted updates walk
all nnz lookups and would see the stale head.  Rates: profiles/graph_forward/ragged_rates.md.

Fused lookup + interaction.  Inside a capture nothing can ask the device whether offsets == arange(B); the proof is made per request on
the caller's tensors (ops.offsets_are_iota: cached per tensor object, free for producer-tagged tensors), only for models that have a fused
route at all, and its verdict is part of the graph's key: a request that fails it runs the graph captured with the two-kernel form.  The
verdict reaches the captured forward through the proof's own cache, set on the STATIC offsets tensors this object owns — the model's
fuse_emb_interact is never touched.

Staleness.  A graph holds raw pointers.  Every call compares the model's table kind, quantize_bits, quantize_mlp_bits, bf16 flag and the
first and last data_ptr of the tensors the forward reads with what the captures saw; a difference drops every graph (`invalidate()`
does the same on request).  In-place weight updates need nothing.

Index errors surface exactly as eager: at the next call's ops.check_index_errors().  When one does, the index buffers of every bucket are
zeroed before the error is raised, so a bad id never stays behind in tail rows.
"""
from __future__ import annotations

import collections
import contextlib
import sys
import weakref
from typing import Optional, Sequence, Tuple

import torch

from . import ext_dist, ops
from .graph_core import (STAGE_MEMCPY_MAX, STAGE_SEGS_PER_LAUNCH, Capture, InFlight, RaggedPlan, StagePlan,  # noqa: F401  (the constants
                         _clone_struct, replay, stage)                                   # and the plans stay importable from here)


# ------------------------------------------------------------------------------------------------ host logic (no device needed)
def pick_bucket(n: int, batch_sizes: Optional[Sequence[int]]) -> Optional[int]:
    """the smallest bucket >= n; None: no buckets, or n above the largest (an exact-shape graph)"""
    best = None
    for b in batch_sizes or ():
        if b >= n and (best is None or b < best):
            best = b
    return best


def _is_stacked(lS_o, lS_i) -> bool:
    so, si = isinstance(lS_o, torch.Tensor), isinstance(lS_i, torch.Tensor)
    if so != si or (so and (lS_o.dim() != 2 or lS_i.dim() != 2 or lS_o.size(0) != lS_i.size(0))):
        raise RuntimeError("dlrm_amd.graph: offsets and indices must both be lists of 1-D tensors or both stacked [T, n] tensors")
    if not so and len(lS_o) != len(lS_i):
        raise RuntimeError("dlrm_amd.graph: offsets / indices table counts differ")
    return so


_steps_cache: dict = {}      # id(offsets tensor) -> (weakref, _version, P, verdict): offsets == P * arange, as iota.py caches P == 1


def _offsets_are_steps(o: torch.Tensor, P) -> bool:
    """o (1-D, or stacked [T, n] with P a tuple) == P * arange(n): one comparison on the tensor's device + a host wait, once per tensor object"""
    e = _steps_cache.get(id(o))
    if e is not None and e[0]() is o and e[1] == o._version and e[2] == P:
        return e[3]
    n = o.size(-1)
    step = torch.arange(n, dtype=o.dtype, device=o.device)
    if o.dim() == 2:
        want = step.unsqueeze(0) * torch.tensor(P, dtype=o.dtype, device=o.device).unsqueeze(1)
    else:
        want = step * P
    ok = bool(torch.equal(o, want))
    if len(_steps_cache) > 256:
        for k in [k for k, v in _steps_cache.items() if v[0]() is None]:
            del _steps_cache[k]
        if len(_steps_cache) > 256:
            _steps_cache.clear()
    _steps_cache[id(o)] = (weakref.ref(o), o._version, P, ok)
    return ok


def fixed_bag_lengths(lS_o, lS_i, n: int) -> Optional[Tuple[int, ...]]:
    """(P_0, ..., P_{T-1}) when table k has exactly P_k >= 1 lookups in every one of its n bags (numel(indices_k) == P_k * n and
    offsets_k == P_k * arange(n)), else None.  What a bucket needs: the static offsets of the padded batch are then P_k * arange(bucket).
    All P_k == 1 on the GPU is the library's one-lookup-per-bag proof (ops.offsets_are_iota: producer tags, cached verdicts)."""
    stacked = _is_stacked(lS_o, lS_i)
    if n <= 0:
        return None
    T = lS_o.size(0) if stacked else len(lS_o)
    Ps = []
    for k in range(T):
        no, ni = (lS_o.size(1), lS_i.size(1)) if stacked else (lS_o[k].numel(), lS_i[k].numel())
        if no != n or ni < n or ni % n != 0:
            return None
        Ps.append(ni // n)
    Ps = tuple(Ps)
    on_gpu = lS_o.is_cuda if stacked else all(o.is_cuda for o in lS_o)
    if on_gpu and all(p == 1 for p in Ps):
        return Ps if ops.offsets_are_iota(lS_o) else None
    if stacked:
        return Ps if _offsets_are_steps(lS_o, Ps) else None
    return Ps if all(_offsets_are_steps(o, p) for o, p in zip(lS_o, Ps)) else None


def alias_pattern(ts) -> Optional[tuple]:
    """None when every tensor of the list is its own object, else for each position the first position holding the same object (a request
    that shares ONE offsets tensor among its tables is staged once, into one static tensor)"""
    first, out, shared = {}, [], False
    for k, t in enumerate(ts):
        j = first.setdefault(id(t), k)
        shared |= j != k
        out.append(j)
    return tuple(out) if shared else None


def lookup_capacities(lookup_capacity, T: Optional[int] = None) -> Optional[Tuple[int, ...]]:
    """the constructor's `lookup_capacity` as (c_0, ..., c_{T-1}): an int holds for every table (a 1-tuple until T is known), a sequence
    names each table's; ValueError for anything that is not an int >= 1, or a sequence of another length than T"""
    if lookup_capacity is None:
        return None
    seq = isinstance(lookup_capacity, (list, tuple))
    cs = tuple(lookup_capacity) if seq else (lookup_capacity,)
    if not cs or any(isinstance(c, bool) or not isinstance(c, int) or c < 1 for c in cs):
        raise ValueError("dlrm_amd.graph: lookup_capacity is an int >= 1 or a sequence of one int >= 1 per table")
    if T is None:
        return cs
    if not seq:
        return cs * T
    if len(cs) != T:
        raise ValueError("dlrm_amd.graph: lookup_capacity names %d tables, the request has %d" % (len(cs), T))
    return cs


def ragged_fits(lS_o, lS_i, n: int, lcaps: Sequence[int]) -> bool:
    """does a request of n rows go into a ragged bucket whose table k holds lcaps[k] lookups?  Every table has n offsets and at most
    lcaps[k] ids, offsets and ids share one int32 / int64 dtype; stacked inputs need ONE capacity; tables that share a tensor object
    (one offsets tensor for all tables) need the same nnz and the same capacity — the shared static buffer has one shift."""
    stacked = _is_stacked(lS_o, lS_i)
    if n < 1:
        return False
    if stacked:
        return (lS_o.size(0) == len(lcaps) and len(set(lcaps)) == 1 and lS_o.size(1) == n and lS_i.size(1) <= lcaps[0]
                and lS_i.dtype == lS_o.dtype and lS_i.dtype in (torch.int32, torch.int64))
    T = len(lS_i)
    if T != len(lcaps) or T == 0:
        return False
    idt = lS_i[0].dtype
    if idt not in (torch.int32, torch.int64):
        return False
    for k in range(T):
        o, i = lS_o[k], lS_i[k]
        if o.dim() != 1 or i.dim() != 1 or o.numel() != n or i.numel() > lcaps[k] or o.dtype != idt or i.dtype != idt:
            return False
    for pattern in (alias_pattern(lS_o), alias_pattern(lS_i)):
        for k, j in enumerate(pattern or ()):
            if j != k and (lS_i[j].numel() != lS_i[k].numel() or lcaps[j] != lcaps[k]):
                return False
    return True


class LRU:
    """key -> value, at most `cap` entries; put() returns the values that fell out (least recently used first)"""

    def __init__(self, cap: int):
        self.cap = max(int(cap), 1)
        self._d: "collections.OrderedDict" = collections.OrderedDict()

    def get(self, key):
        v = self._d.get(key)
        if v is not None:
            self._d.move_to_end(key)
        return v

    def put(self, key, value) -> list:
        self._d[key] = value
        self._d.move_to_end(key)
        out = []
        while len(self._d) > self.cap:
            out.append(self._d.popitem(last=False)[1])
        return out

    def values(self):
        return list(self._d.values())

    def keys(self):
        return list(self._d.keys())

    def clear(self) -> None:
        self._d.clear()

    def __len__(self) -> int:
        return len(self._d)


def model_tensors(model) -> list:
    """the tensors a forward reads through raw pointers: the tables (packed ones first), then every parameter, then the towers' packed
    int8 weights"""
    out = []
    if getattr(model, "quantize_emb", False):
        out += [t for t in (getattr(model, "emb_l_q", None) or []) if isinstance(t, torch.Tensor)]
    out += list(model.parameters())
    for name in ("bot_l", "top_l"):
        tower = getattr(model, name, None)
        tower = getattr(tower, "module", tower)
        for q in getattr(tower, "_q8", None) or []:
            out += [t for t in (q if isinstance(q, (tuple, list)) else [q]) if isinstance(t, torch.Tensor)]
    return out


def model_scalars(model) -> tuple:
    kind = model._table_kind() if hasattr(model, "_table_kind") else None
    return (kind, getattr(model, "quantize_bits", None), getattr(model, "quantize_mlp_bits", 32), getattr(model, "emb_bf16", None) is not None)


def fingerprint(model, tensors: Sequence) -> tuple:
    """the cheap per-call form: the scalars plus the first and last pointer of `tensors` (model_tensors at the time of the captures)"""
    if not tensors:
        return model_scalars(model) + (0, 0)
    return model_scalars(model) + (tensors[0].data_ptr(), tensors[-1].data_ptr())


class _Graph(Capture):
    """one captured forward: the capture plus its key, static inputs and plan"""
    __slots__ = ("key", "bucket", "n", "static", "plan", "eager_calls", "views", "iota")

    def __init__(self, key, bucket, n, stream):
        super().__init__(stream)
        self.key, self.bucket, self.n = key, bucket, n
        self.static = self.plan = None
        self.eager_calls = 0
        self.views = {}
        self.iota = None          # the offsets verdict the forward on the static buffers runs with (None: no fused route asks)


# ------------------------------------------------------------------------------------------------ the class
class GraphedForward:
    """fwd = GraphedForward(model, batch_sizes=None, warmup=2, lookup_capacity=None);  Z = fwd(X, lS_o, lS_i)   ([n, 1] view of a static
    buffer).  lookup_capacity (an int, or one int per table; needs batch_sizes): ragged multi-hot requests run in ragged buckets of
    bucket * c_k lookups for table k (module docstring); None: they take exact-shape graphs.

    The first `warmup` calls of a graph are eager forwards on its static buffers (kernel attributes, workspaces and allocator pools
    settle; a bucket answers with the padded batch's bits from its first call on); the next call captures, every later one stages and
    replays.  Counters: captures, replays, staged_launches (dlrm_stage_inputs / dlrm_stage_ragged kernel launches of the replays; the
    memcpy path adds none), buckets_in_use (bucket sizes with a captured graph, of either kind), ragged_buckets_in_use."""

    def __init__(self, model, batch_sizes: Optional[Sequence[int]] = None, warmup: int = 2, max_exact_shapes: int = 8,
                 lookup_capacity=None):
        if ext_dist.is_distributed():
            raise RuntimeError("dlrm_amd.graph: the whole-forward HIP graph is single-process only "
                               "(the RCCL all-to-all of the distributed forward is not captured)")
        self.batch_sizes = tuple(sorted({int(b) for b in batch_sizes})) if batch_sizes else None
        if self.batch_sizes and self.batch_sizes[0] < 1:
            raise ValueError("dlrm_amd.graph: batch_sizes must be positive")
        self.lookup_capacity = lookup_capacities(lookup_capacity)
        if self.lookup_capacity is not None and not self.batch_sizes:
            raise ValueError("dlrm_amd.graph: lookup_capacity sizes the ragged buckets; it needs batch_sizes")
        self._lookup_capacity_arg = lookup_capacity
        self.model = model
        self._refuse_int8_buckets()
        self.warmup = max(int(warmup), 1)
        self.stream: Optional[torch.cuda.Stream] = None
        self.stage_memcpy_max = STAGE_MEMCPY_MAX
        self.flight = InFlight()    # one replay in flight
        self._exact = LRU(max_exact_shapes)
        self._buckets: dict = {}
        self._keep = None
        self._tensors: list = []
        self._fp = None
        self._route = False
        self.captures = 0
        self.replays = 0
        self.staged_launches = 0

    # ---- refusals, staleness ------------------------------------------------------------------------------------------------------
    def _refuse_int8_buckets(self) -> None:
        if self.batch_sizes and getattr(self.model, "quantize_mlp_bits", 32) == 8:
            sys.exit("ERROR: GraphedForward with batch_sizes: int8 towers quantise per batch; padded buckets would change the result "
                     "(exact-shape graphs work: batch_sizes=None)")

    @property
    def buckets_in_use(self) -> int:
        return len({g.bucket for g in self._buckets.values() if g.graph is not None})

    @property
    def ragged_buckets_in_use(self) -> int:
        return len({g.bucket for g in self._buckets.values() if g.graph is not None and g.key[0] == "ragged"})

    @property
    def exact_shapes(self) -> int:
        return len(self._exact)

    def invalidate(self) -> None:
        """forget every captured graph (the next calls capture again) — after anything that moved a tensor the forward reads"""
        self._wait()
        for g in self._exact.values() + list(self._buckets.values()):
            g.reset()
        self._exact.clear()
        self._buckets.clear()
        self._keep = None
        self._fp = None

    def _refresh(self) -> None:
        """what the captures depend on, taken from the model as it is now"""
        model = self.model
        self._refuse_int8_buckets()
        self._tensors = model_tensors(model)
        self._fp = fingerprint(model, self._tensors)
        self._route = self._has_fused_route()

    def _has_fused_route(self) -> bool:
        """does this model have fused lookup + interaction kernels at all (dlrm_net.fused_route, asked as DLRM_Net._fused_forward asks under
        no_grad)?  Only then is a request's offsets proof worth its host wait."""
        m = self.model
        if not (getattr(m, "fuse_emb_interact", False) and hasattr(m, "fused_route_now")):
            return False
        from .dlrm_net import DLRM_Net
        if type(m).sequential_forward is not DLRM_Net.sequential_forward:
            return False                      # (the cat-interaction variants bring their own forward: no route)
        return m.fused_route_now() is not None

    # ---- helpers -------------------------------------------------------------------------------------------------------------------
    def _wait(self) -> None:
        self.flight.wait(torch.cuda.current_stream())

    def _check_errors(self) -> None:
        """ops.check_index_errors() as the eager forward calls it.  A reported id may still sit in a bucket's rows, and a request replayed
        since — before the report was seen — may have met it there again and reported it once more: everything enqueued is waited for, the
        index rows of every bucket are zeroed, and what the error block received meanwhile is dropped where it is the same bad id (another
        one is reported in the same exception), so that ONE bad request raises ONCE and no later request answers for it."""
        try:
            ops.check_index_errors()
        except IndexError as first:
            self.flight.wait(torch.cuda.current_stream(), always=True)
            second = None
            try:
                ops.check_index_errors()
            except IndexError as e:
                if str(e) != str(first):            # (another bad id, of a request replayed since: reported with this one, not lost)
                    second = e
            for g in self._buckets.values():
                seen = set()
                for t in ([g.static[2]] if isinstance(g.static[2], torch.Tensor) else g.static[2]):
                    if id(t) not in seen:
                        seen.add(id(t))
                        t.zero_()
            if second is not None:
                raise IndexError("%s; and, from a request replayed since: %s" % (first, second)) from first
            raise

    @contextlib.contextmanager
    def _single_stream(self):
        """the captured forward is single-stream (a replayed graph has no launch gaps to hide); the model's own setting comes back"""
        model = self.model
        was = getattr(model, "overlap_streams", False)
        if was:
            model.overlap_streams = False
        try:
            yield
        finally:
            if was:
                model.overlap_streams = True

    def _normalise(self, X, lS_o, lS_i, dev):
        def fix(t):
            if t.device != dev:
                t = t.to(dev)
            return t if t.is_contiguous() else t.contiguous()
        X = fix(X)
        if isinstance(lS_o, torch.Tensor):
            return X, fix(lS_o), fix(lS_i)
        fixed = {}
        return X, [fixed.setdefault(id(t), fix(t)) for t in lS_o], [fixed.setdefault(id(t), fix(t)) for t in lS_i]

    def _lookup(self, X, lS_o, lS_i):
        """-> the graph this request runs in (made on first sight)"""
        stacked = _is_stacked(lS_o, lS_i)
        n = X.size(0)
        bucket = pick_bucket(n, self.batch_sizes)
        Ps = fixed_bag_lengths(lS_o, lS_i, n) if bucket is not None else None
        idt = lS_i.dtype if stacked else lS_i[0].dtype
        if Ps is not None:
            T = len(Ps)
            key = ("bucket", bucket, stacked, X.size(1), X.dtype, idt, Ps, None if stacked else alias_pattern(lS_i))
            g = self._buckets.get(key)
            if g is None:
                dev = X.device
                g = self._buckets[key] = _Graph(key, bucket, bucket, self.stream)
                Xs = torch.zeros((bucket, X.size(1)), dtype=X.dtype, device=dev)
                step = torch.arange(bucket, dtype=idt, device=dev)
                if stacked:
                    Os = step.unsqueeze(0) * torch.tensor(Ps, dtype=idt, device=dev).unsqueeze(1)
                    Is = torch.zeros((T, bucket * Ps[0]), dtype=idt, device=dev)
                else:
                    Os = [step * p for p in Ps]
                    made = {}
                    Is = [made.setdefault(id(t), torch.zeros(bucket * p, dtype=idt, device=dev)) for t, p in zip(lS_i, Ps)]
                g.static = (Xs, Os, Is)
                # (stacked ids go in by rows whatever this first request's width: the next one of the key may be narrower)
                g.plan = StagePlan((Xs, None, Is), (X, lS_o, lS_i), by_rows=(2,) if stacked else ())
                g.iota = all(p == 1 for p in Ps)
            return g
        if bucket is not None and self.lookup_capacity is not None:
            g = self._ragged(X, lS_o, lS_i, stacked, n, bucket, idt)
            if g is not None:
                return g
        # exact shape.  The offsets' verdict is part of the key where the model could take a fused route with these shapes
        if stacked:
            shape = (tuple(lS_o.shape), tuple(lS_i.shape))
            one = lS_o.size(1) == n and lS_i.size(1) == n
        else:
            no, ni = [o.numel() for o in lS_o], [i.numel() for i in lS_i]
            shape = (tuple(no), tuple(ni), alias_pattern(lS_o), alias_pattern(lS_i))
            one = no.count(n) == len(no) and ni.count(n) == len(ni)
        iota = bool(ops.offsets_are_iota(lS_o)) if (self._route and one and n > 0) else None
        key = ("exact", stacked, tuple(X.shape), X.dtype, idt, shape, iota)
        g = self._exact.get(key)
        if g is None:
            g = _Graph(key, None, n, self.stream)
            g.static = (X.clone(), _clone_struct(lS_o), _clone_struct(lS_i))
            g.plan = StagePlan(g.static, (X, lS_o, lS_i))
            g.iota = iota
            dropped = self._exact.put(key, g)
            if dropped:
                self._wait()
                for d in dropped:
                    d.reset()
        return g

    def _ragged(self, X, lS_o, lS_i, stacked, n, bucket, idt):
        """-> the ragged bucket of this request, or None: it does not fit one (an exact-shape graph).  The static ids of table k hold
        Lcap_k = bucket * c_k lookups, the request's at their END; the static offsets are rewritten by every request (RaggedPlan)."""
        T = lS_o.size(0) if stacked else len(lS_o)
        caps = lookup_capacities(self._lookup_capacity_arg, T)
        lcaps = tuple(bucket * c for c in caps)
        if X.dim() != 2 or not ragged_fits(lS_o, lS_i, n, lcaps):
            return None
        key = ("ragged", bucket, stacked, X.size(1), X.dtype, idt, caps, None if stacked else (alias_pattern(lS_o), alias_pattern(lS_i)))
        g = self._buckets.get(key)
        if g is None:
            dev = X.device
            g = self._buckets[key] = _Graph(key, bucket, bucket, self.stream)
            Xs = torch.zeros((bucket, X.size(1)), dtype=X.dtype, device=dev)
            if stacked:
                Os = torch.full((T, bucket), lcaps[0], dtype=idt, device=dev)
                Is = torch.zeros((T, lcaps[0]), dtype=idt, device=dev)
            else:
                mo, mi = {}, {}         # (one tensor object at several positions: one static buffer)
                Os = [mo[id(t)] if id(t) in mo else mo.setdefault(id(t), torch.full((bucket,), L, dtype=idt, device=dev))
                      for t, L in zip(lS_o, lcaps)]
                Is = [mi[id(t)] if id(t) in mi else mi.setdefault(id(t), torch.zeros(L, dtype=idt, device=dev)) for t, L in zip(lS_i, lcaps)]
            g.static = (Xs, Os, Is)
            g.plan = RaggedPlan(g.static, lcaps, bucket)
            # Lcap_k == bucket for every table is the shape the fused lookup + interaction kernels take, and a captured forward must not
            # ask the device about offsets: stated "not arange" (a request that IS arange went to its fixed-length bucket above), so the
            # capture holds the two-kernel form.  Any other capacity never reaches that question (nnz != B).
            g.iota = False if (self._route and all(L == bucket for L in lcaps)) else None
        return g

    @staticmethod
    def _vouch(g: _Graph) -> None:
        """the verdict of the offsets proof, stated for the STATIC offsets tensors (iota.vouch_offsets): the forward run or captured on them
        takes the fused kernels alone (True) or the two-kernel form (False).  Stated in front of EVERY forward on the static buffers — the
        record is a cache entry that other proofs can evict — and true whenever it is stated: every request is proven before it is staged."""
        if g.iota is None:
            return
        from . import iota as _iota
        static_o = g.static[1]
        for t in ([static_o] if isinstance(static_o, torch.Tensor) else static_o):
            _iota.vouch_offsets(t, g.iota)

    def _forward(self, g: _Graph, dev, how):
        """the model's forward on the static buffers through g.run (warm-up) or g.record (capture)"""
        self._vouch(g)
        with self._single_stream(), torch.no_grad():
            return how(dev, lambda: self.model(*g.static))

    def _capture(self, g: _Graph, dev) -> None:
        Z = self._forward(g, dev, g.record)
        if Z.dim() != 2 or Z.size(0) != g.n or not Z.is_contiguous():
            g.reset()
            raise RuntimeError("dlrm_amd.graph: the captured forward returned %s, expected a contiguous [%d, k] tensor" % (tuple(Z.shape), g.n))
        g.out, g.views = Z.detach(), {}
        self.captures += 1

    # ---- the call ------------------------------------------------------------------------------------------------------------------
    def __call__(self, X, lS_o, lS_i):
        self._check_errors()
        model = self.model
        if self._fp is None or fingerprint(model, self._tensors) != self._fp:
            if self._fp is not None:
                self.invalidate()
            self._refresh()
        dev = self._tensors[0].device if self._tensors else X.device
        if dev.type != "cuda":
            raise RuntimeError("dlrm_amd.graph: GraphedForward captures a HIP graph; move the model to the GPU first (model.to('cuda'))")
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)     # ONE capture stream for every graph: the scratch workspaces are per stream
        X, lS_o, lS_i = self._normalise(X, lS_o, lS_i, dev)
        n = X.size(0)
        g = self._lookup(X, lS_o, lS_i)
        request = (X, lS_o, lS_i)
        if g.graph is None:
            self._wait()
            self._check_errors()            # (exact for everything this object enqueued: nothing of it is in flight any more)
            if g.eager_calls < self.warmup:
                stage(g.plan, request, torch.cuda.current_stream())
                g.out = self._forward(g, dev, g.run)
                g.out.record_stream(torch.cuda.current_stream(dev))
                g.eager_calls += 1
                self._keep = request
                return g.out if g.bucket is None else g.out[:n]
            self._capture(g, dev)           # capture only records; the replay below executes this request
        raw = g.exec is not None
        replay(g, self.flight, torch.cuda.current_stream(), g.plan, request, memcpy_max=self.stage_memcpy_max)
        self.staged_launches += g.plan.launches(self.stage_memcpy_max if raw else 0)
        self.replays += 1
        self._keep = request                # the sources stay alive until the next call (their copies are asynchronous)
        if g.bucket is None:
            return g.out
        z = g.views.get(n)
        if z is None:
            z = g.views[n] = g.out[:n]
        return z

