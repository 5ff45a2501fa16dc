"""The "one lookup per bag" proof in front of the fused lookup + interaction path (reached through dlrm_amd.ops, which re-exports it)."""
# nnz == B does not prove offsets == arange(B): EmbeddingBag accepts an empty bag next to a two-lookup bag (dlrm_s_pytorch.py:453-457) and
# the reference computes that input correctly.  The proof is one pass over the offsets on the device, paid once per distinct offsets tensor:
# the verdict is cached on the tensor OBJECT (weak reference, so a recycled address can never alias) together with its in-place version
# counter.  Two forms: the host waits for the verdict (offsets_are_iota_start / _finish), or the verdict stays on the device as a launch
# predicate (offsets_iota_state, the default) and the host looks at its pinned mirror whenever a later call finds the proof's event complete.
#
# Who keeps the flag words alive (all of them belong to the per-device _State below):
#   1. a pending device proof holds its _FlagPool (device words + pinned mirrors) and is dropped only once its event has completed;
#   2. the pending list is bounded by forgetting old entries' weak references (their verdict is not remembered), never the entries;
#   3. a flag handed out carries the stream its pool was allocated under (`flag.dlrm_pool_stream`); a launch that uses the flag on ANOTHER
#      stream calls flag.record_stream first (here and in ops._pred_args), so a retired pool is not re-used before that launch has run;
#   4. on its own stream the pool needs no more: the consumers hold the flag until they are enqueued, the allocator orders re-use behind them;
#   5. the host proof's pinned flag returns to the free list in offsets_are_iota_finish only, after the event behind its check kernel.
import collections
import ctypes as C
import time
import weakref

import torch

from . import _lib, ops          # (ops imports this module at its END: _timed, _stream, wait_spinning are looked up when called)

IOTA_STATS = {"checked": 0, "cached": 0, "tagged": 0, "device_predicates": 0, "host_us": 0.0, "wait_us": 0.0}
_IOTA_TAG = "_dlrm_one_lookup_per_bag"      # attribute a PRODUCER sets on an offsets tensor it wrote as 0, 1, ..., B-1
_iota_cache: dict = {}                      # id(tensor) -> (weakref, _version, verdict)


def mark_one_lookup_per_bag(t: torch.Tensor) -> torch.Tensor:
    """Producer-side proof: whoever WROTE the bag starts as 0, 1, ..., B-1 (dlrm_amd.datagen with one fixed lookup per bag,
    CriteoBinBatches, Multihot over all-ones hot sizes — by construction of their kernels) tags the tensor object, and
    `offsets_are_iota` then needs neither a device pass nor a synchronisation for it.  The tag holds the tensor's in-place version
    counter, so a later versioned write voids it; views and copies are new objects and carry no tag (they take the device proof) — and
    because Python attributes DO travel with copy.deepcopy / pickle, the tag also names the object and the storage address it was given
    for: a deep copy or an unpickled tensor is a different object at a different address and is therefore untagged.  What no tag
    can see is a write that bypasses the version counter (`.data` writes, a foreign kernel): producers tag tensors their own kernel has just
    written and hand them over; the fused kernels still verify every bag start they use and report a violation through the error block."""
    setattr(t, _IOTA_TAG, (t._version, id(t), t.data_ptr()))
    return t


def _iota_tagged(t: torch.Tensor) -> bool:
    return getattr(t, _IOTA_TAG, None) == (t._version, id(t), t.data_ptr())


def _iota_cached(t: torch.Tensor):
    e = _iota_cache.get(id(t))
    if e is not None and e[0]() is t and e[1] == t._version:
        return e[2]
    return None


def _iota_remember(t: torch.Tensor, verdict: bool) -> None:
    if len(_iota_cache) > 256:
        for k in [k for k, e in _iota_cache.items() if e[0]() is None]:
            del _iota_cache[k]
        if len(_iota_cache) > 256:
            _iota_cache.clear()
    _iota_cache[id(t)] = (weakref.ref(t), t._version, verdict)


def vouch_offsets(t: torch.Tensor, verdict: bool) -> None:
    """The owner of an offsets tensor states the verdict a proof would reach — for tensors written through raw pointers only (the static
    offsets buffers of dlrm_amd.graph.GraphedForward, whose every request is proven before it is staged): recorded like a finished proof,
    per tensor object and in-place version.  The record is a cache entry and can be evicted (_iota_remember): state it again in front of
    every use that depends on it."""
    _iota_remember(t, bool(verdict))


POOL_SLOTS = 1024
PENDING_REMEMBERED = 64      # device proofs whose verdict is still wanted: one nobody came back for within 64 steps is not remembered


class _FlagPool:
    """device int32 words + their pinned mirrors; a slot is used ONCE (zeroed at allocation, never re-armed)"""
    __slots__ = ("dev", "host", "next", "stream")

    def __init__(self, device):
        self.dev = torch.zeros(POOL_SLOTS, dtype=torch.int32, device=device)
        self.host = torch.zeros(POOL_SLOTS, dtype=torch.int32).pin_memory()
        self.next = 0
        self.stream = torch.cuda.current_stream(device).cuda_stream       # what the caching allocator orders re-use of `dev` by


# a device proof whose host-visible verdict (pool.host[slot]) has not been looked at yet: `event` follows its kernel, `refs` is the list of weak
# references to the tensor objects the verdict is for
_Pending = collections.namedtuple("_Pending", "event pool slot refs")


class _State:
    """what the proofs own on one device"""
    __slots__ = ("proof_stream", "free_flags", "pool", "pending")

    def __init__(self):
        self.proof_stream = None     # the (high-priority) stream the host proof's check kernels run on
        self.free_flags = []         # pinned int32[1] flags of finished host proofs
        self.pool = None             # the _FlagPool the next device proof takes its slot from
        self.pending = []            # [_Pending]


_states = collections.defaultdict(_State)      # device index -> _State


def _drain(pending: list) -> None:
    """remember the verdicts of finished device proofs (event.query(): no wait) — a tensor object that comes back is then known"""
    keep = []
    for p in pending:
        if p.event.query():
            ok = int(p.pool.host[p.slot]) == 0
            for r in p.refs:                   # (weak references: the proof keeps no offsets tensor alive; an object that is gone needs no verdict)
                t = r()
                if t is not None:
                    _iota_remember(t, ok)
        else:
            keep.append(p)
    for p in keep[:-PENDING_REMEMBERED]:       # (the next encounter of these tensors proves again; the entry stays until its kernel has run)
        p.refs.clear()
    pending[:] = keep


class _IotaProof:
    """A proof about to be launched: the arguments of the check kernel; `keep` holds the (contiguous) tensors behind `ptrs`.  The host
    proof hands it out as its handle: the check kernel runs on the proof stream behind an event of the caller's stream recorded when the
    proof was requested; `done` fires when the verdict is in `flag` (pinned host memory the kernel counts violations into)."""
    __slots__ = ("t0", "srcs", "keep", "n", "ptrs", "B", "bits", "dev", "flag", "done")


def _prepare(lS_o):
    """The front half of both proofs: True / False when the verdict is known (producer tag, cached per tensor object), None while a
    HIP graph is being captured (undecided: GraphedTrainStep proves every incoming batch before the replay), else an _IotaProof."""
    srcs = [lS_o] if isinstance(lS_o, torch.Tensor) else list(lS_o)
    if all(_iota_tagged(t) for t in srcs):
        IOTA_STATS["tagged"] += 1
        return True
    verdicts = [True if _iota_tagged(t) else _iota_cached(t) for t in srcs]
    if all(v is not None for v in verdicts):
        IOTA_STATS["cached"] += 1
        return all(verdicts)
    if torch.cuda.is_current_stream_capturing():
        return None
    a = _IotaProof()
    a.t0 = time.perf_counter()
    ptrs, a.keep = [], []
    for t in srcs:
        if not t.is_cuda or t.dtype not in (torch.int64, torch.int32) or t.dtype != srcs[0].dtype:
            raise RuntimeError("dlrm_amd: offsets must be int32/int64 GPU tensors of one dtype")
        if t.dim() == 2:
            if t.stride(1) != 1 and t.size(1) > 1:
                t = t.contiguous()
            ptrs += [t.data_ptr() + k * t.stride(0) * t.element_size() for k in range(t.size(0))]
        else:
            t = t.contiguous()
            ptrs.append(t.data_ptr())
        a.keep.append(t)
    a.srcs, a.n, a.ptrs, a.B = srcs, len(ptrs), _lib.ptr_array(ptrs), srcs[0].size(-1)
    a.bits, a.dev = 64 if srcs[0].dtype == torch.int64 else 32, srcs[0].device
    return a


# ---- the host waits for the verdict (DLRM_DEVICE_PREDICATE=0, GraphedTrainStep) ----------------------------------------------------------
def offsets_are_iota_start(lS_o):
    """First half of the proof.  Returns True / False / None as _prepare does, else a handle for `offsets_are_iota_finish`.  The check
    kernel is NOT put on the caller's stream: it runs on a proof stream that waits only for what the caller's stream holds at this
    moment (the tensor's producer, by torch's stream convention), so everything the caller enqueues AFTER this call — DLRM_Net runs the
    whole bottom tower here — is queued behind nothing of the proof and keeps the GPU busy while the host waits for the verdict."""
    h = _prepare(lS_o)
    if not isinstance(h, _IotaProof):
        return h
    st = _states[h.dev.index]
    h.flag = st.free_flags.pop() if st.free_flags else torch.zeros(1, dtype=torch.int32).pin_memory()
    h.flag[0] = 0
    if st.proof_stream is None:
        st.proof_stream = torch.cuda.Stream(device=h.dev, priority=-1)
    st.proof_stream.wait_event(torch.cuda.current_stream(h.dev).record_event())
    rc = _lib.load().dlrm_offsets_are_iota(h.n, h.B, h.ptrs, h.bits, C.c_void_p(h.flag.data_ptr()), C.c_void_p(st.proof_stream.cuda_stream))
    _lib.check(rc, "dlrm_offsets_are_iota")
    h.done = st.proof_stream.record_event()
    IOTA_STATS["host_us"] += (time.perf_counter() - h.t0) * 1e6
    return h


def offsets_are_iota_finish(h) -> bool:
    """Second half: wait for the check kernel alone (an event of the proof stream, not a stream synchronisation of the caller's) and
    read the verdict.  The offsets tensors stayed alive in the handle until here."""
    if not isinstance(h, _IotaProof):
        return h
    t0 = time.perf_counter()
    ops.wait_spinning(h.done)
    ok = int(h.flag[0]) == 0
    _states[h.dev.index].free_flags.append(h.flag)
    IOTA_STATS["checked"] += 1
    # one verdict for the whole set: each tensor of a list is remembered with it (a False verdict of the set is re-examined only if
    # the same objects come back, and then it is False again)
    for t in h.srcs:
        _iota_remember(t, ok)
    IOTA_STATS["wait_us"] += (time.perf_counter() - t0) * 1e6
    h.keep = h.srcs = None
    return ok


def offsets_are_iota(lS_o):
    """True iff every table's bag starts are 0, 1, ..., B-1 (with nnz == B: exactly one lookup per bag).  `lS_o` is what the caller
    passed to the module (a stacked [T, B] tensor or a list of [B] tensors).  Free for tensors their PRODUCER tagged
    (`mark_one_lookup_per_bag`: dlrm_amd.datagen, CriteoBinBatches, Multihot know it by construction) and for tensor objects seen
    before (verdict cached per object + in-place version; a write that does not bump `_version` — `t.data.copy_`, a collective or a
    custom kernel writing into a reused buffer — is not noticed here: the fused kernels still verify every bag start themselves and
    report a violation through the index-error block, so reused offsets buffers must be updated through versioned in-place ops).
    Any other tensor takes one device pass + a host wait for it (`offsets_are_iota_start` / `_finish`).  While a HIP graph is being
    captured no wait is possible: returns None (undecided) — GraphedTrainStep proves the incoming batch before every replay."""
    return offsets_are_iota_finish(offsets_are_iota_start(lS_o))


# ---- the verdict left on the DEVICE (ABI 16): no host wait at all -------------------------------------------------------------------------
def offsets_iota_state(lS_o):
    """What the caller of the fused lookup + interaction path needs to know about `lS_o`, WITHOUT waiting for the device:
      True / False    the verdict is known (producer tag, or this tensor object was proven earlier);
      None            a HIP graph is being captured (undecided: GraphedTrainStep proves every incoming batch before the replay);
      a device int32  the proof was enqueued on the CURRENT stream (dlrm_offsets_iota_flags: number of bags whose start differs from their
                      number) — the caller enqueues both implementations with that launch predicate (functional.gather_interact_fwd) and never
                      waits; the host-visible copy of the verdict is looked at whenever a later call finds its event complete."""
    for st in _states.values():
        _drain(st.pending)
    a = _prepare(lS_o)
    if not isinstance(a, _IotaProof):
        return a
    st = _states[a.dev.index]
    pool = st.pool
    if pool is None or pool.next >= POOL_SLOTS:
        pool = st.pool = _FlagPool(a.dev)
    k = pool.next
    pool.next = k + 1
    flag = pool.dev[k:k + 1]
    flag.dlrm_pool_stream = pool.stream
    cur = torch.cuda.current_stream(a.dev)
    if cur.cuda_stream != pool.stream:
        flag.record_stream(cur)
    with ops._timed("iota_proof"):
        rc = _lib.load().dlrm_offsets_iota_flags(a.n, a.B, a.ptrs, a.bits, C.c_void_p(flag.data_ptr()),
                                                 C.c_void_p(pool.host[k:k + 1].data_ptr()), ops._stream(a.srcs[0]))
    _lib.check(rc, "dlrm_offsets_iota_flags")
    st.pending.append(_Pending(cur.record_event(), pool, k, [weakref.ref(t) for t in a.srcs]))
    IOTA_STATS["device_predicates"] += 1
    IOTA_STATS["host_us"] += (time.perf_counter() - a.t0) * 1e6
    return flag
