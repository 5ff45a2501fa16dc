"""Whole-step HIP graph: forward + loss + backward + fused embedding update + dense optimizer step captured once
and replayed with one `hipGraphLaunch` per training step.

Why: at Criteo-Kaggle shapes (BASELINE.json configs[1]: B = 2048, D = 16) one step is ~70 kernel launches of a few
microseconds each and the Python/ctypes/autograd host path (~1 ms per step, measured) is the whole step time; at
Criteo-Terabyte shapes the GPU work (9 ms) hides the host path and replay only removes the inter-kernel gaps.
The reference loop body (dlrm_s_pytorch.py:1574-1621) is what gets captured, unchanged in order:
    Z = dlrm(X, lS_o, lS_i); E = loss_fn(Z, T); optimizer.zero_grad(); E.backward(); optimizer.step()

Everything the C ABI enqueues is capture-safe by construction: kernels take table / tensor pointers by value in
the kernarg segment, nothing allocates or synchronises, scratch buffers come from torch's caching allocator (graph
private pool during capture) and the segmented sort of the embedding updates is made of plain kernels on the capture stream.

The mechanics (static inputs, capture stream, the one-replay-in-flight rule, the replay call) are graph_core.py's, shared with
graph_forward.py; here: what is refused, the sort mode, the offsets proof, and the owners DeviceLearningRates and StepStateMirrors.

Constraints (checked, never silently worked around):
  * single process (ext_dist.my_size == 1): RCCL collectives and DDP hooks are not captured;
  * fixed shapes: every call must pass tensors of the shapes/dtypes of the first call (multi-hot batches whose number
    of lookups varies cannot be replayed) — inputs are copied into static device buffers before each replay;
  * no autograd graph of an earlier eager step may still be alive at capture time (e.g. a loss tensor the caller kept):
    the autograd engine would synchronise the capture stream with the stream those old nodes were created on, which
    invalidates the capture.  Reduce losses to Python floats (`float(loss)`) or `del` them before the first graphed call;
  * the GPU memory fault at B = 65536 of round 1 (profiles/r02/graph_probe.md d) came from replaying rocPRIM's radix sort, not from
    the batch size (tools/probes/graph_sorted_probe.py).  The sort-based updates now run on the library's own segmented sorter
    (csrc/seg_sort.h) whenever every table segment holds <= 262144 lookups — then the graph keeps the sorted update and the fused
    row-wise Adagrad; otherwise it switches SGD to the atomic update and refuses the Adagrad update (GraphedTrainStep.
    _settle_sort_mode).  tests/test_gpu_model.py replays 36 full-batch steps with host syncs in between, bit-identical to eager;
  * learning rates (round 6): with this package's optimizers (FusedSGD, FusedRWSAdagrad with lr_decay == 0) every captured update kernel
    reads its step size from a DEVICE scalar (one per param group; include/dlrm_hip.h "LEARNING RATES"), and a replay whose param groups
    carry new lr values writes them in front of the launch (dlrm_graph_replay / dlrm_set_f32: values in the kernarg, no host buffer, no
    synchronisation) — the reference's LRPolicyScheduler, which moves lr EVERY iteration during warm-up and decay
    (dlrm_s_pytorch.py:169-203, :1621), is followed with ONE capture.  Any other optimizer (torch.optim.SGD: its foreach step takes lr as a
    host number) keeps the old rule: lr is baked in at capture time and a change re-captures the step;
  * step state (opt-in: GraphedTrainStep(..., device_step_state=True)): what else changes from step to step moves to the device the way
    the learning rates did.  bfloat16 tables (torch SGD, FusedSGD, FusedRWSAdagrad): the Philox key of every update is drawn by a captured
    dlrm_philox_key_next launch from a device counter of update calls, and the captured *_devkey update kernels read it when they run
    (include/dlrm_hip.h "STEP STATE ON THE DEVICE") — the key sequence of the eager step, bit for bit.  The counter starts, at every capture,
    from model._bf16_update_calls.  The bf16 update is sort-based always: the Adagrad rule of _settle_sort_mode applies (a table segment
    that needs the general sorter raises; nothing is captured), and a captured step that drew other than one key per parked backward pass
    raises.  FusedAdagrad (lr_decay == 0): its kernels read lr from the group's device scalar as the other two optimizers' do.  HOST MIRRORS:
    model._bf16_update_calls and every optimizer.state[p]["step"] the captured step advances are pure functions of the number of replays;
    replays are counted and the counters are brought up to date where someone can observe them — optimizer.state_dict() /
    load_state_dict(), an eager optimizer step or eager bf16 update, _drop_graph, a re-capture (_settle) — never per replay, never with a
    host wait.  Eager bf16 updates between replays move the host counter; the device counter is rewritten in front of the next replay.
    Without the keyword bf16 tables and FusedAdagrad exit as before; QR, mixed-dimension and quantised models, a stock torch.optim.Adagrad
    with model.fused_adagrad (its dense step is torch's) and lr_decay != 0 are refused either way.  The capture stays single-stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os as _os
import sys
import weakref
from typing import List, Optional

import torch

from . import ext_dist, ops
from .graph_core import (Capture, InFlight, StagePlan, TensorOrList, _check_struct, _clone_struct, _copy_struct,  # noqa: F401  (the input
                         replay)                                                   # helpers stay importable from here)
from .graph_forward import GraphedForward  # noqa: F401  (the forward pass on the same core: dlrm_amd/graph_forward.py)

_TRACE = _os.environ.get("DLRM_GTS_TRACE", "0") == "1"


class DeviceLearningRates:
    """Step sizes on the device: one fp32 scalar per param group, read by the captured update kernels (module docstring, "learning
    rates"); for any other optimizer only the values the capture baked in."""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        # (FusedAdagrad gets here only with device_step_state)
        self.on_device = type(optimizer).__name__ in ("FusedSGD", "FusedRWSAdagrad", "FusedAdagrad") and _os.environ.get("DLRM_GTS_DEVICE_LR", "1") == "1"
        self.dev: Optional[torch.Tensor] = None     # [number of param groups at capture time]
        self.values: List[float] = []               # the captured graph runs with these
        self.writes = 0                             # replays that carried new step sizes (observability: tests, bench)

    def current(self) -> List[float]:
        return [float(g["lr"]) for g in self.optimizer.param_groups]

    def valid(self) -> bool:
        """False: re-capture (another number of param groups than the scalars were made for; a host step size baked into the capture)"""
        return len(self.optimizer.param_groups) == len(self.values) and (self.on_device or self.current() == self.values)

    @contextlib.contextmanager
    def capturing(self, dev):
        """Around a capture: the scalars, holding the CURRENT lr, handed to the update kernels (ops._graph_lr) for the duration of the
        capture only, so that an eager step of the same optimizer outside the graph keeps passing its host value"""
        groups = list(self.optimizer.param_groups)
        self.dev = torch.tensor(self.current(), dtype=torch.float32, device=dev) if self.on_device else None
        for i, g in enumerate(groups if self.on_device else ()):
            ops._graph_lr[id(g)] = self.dev[i:i + 1]
        try:
            yield
        finally:
            for g in groups:
                ops._graph_lr.pop(id(g), None)
        self.values = self.current()

    def changed(self):
        """(count, device pointers, values) of the step sizes this replay must write first, or None: every group's value whenever any
        changed (at most 16 go with the replay call, more are written right here); never for another group count than the captured one"""
        if self.dev is None:
            return None
        lrs = self.current()
        n = len(lrs)
        if lrs == self.values or n != self.dev.numel():
            return None
        self.values = lrs
        self.writes += 1
        if n > 16:
            ops.set_f32([self.dev[i:i + 1] for i in range(n)], lrs)
            return None
        base = self.dev.data_ptr()
        return n, (C.c_void_p * n)(*[base + 4 * i for i in range(n)]), (C.c_float * n)(*lrs)


class StepStateMirrors:
    """Step state (device_step_state; module docstring): what ONE replay advances — bf16 key draws and (parameter, state["step"]
    increment) pairs, found at capture time — the replays the host mirrors have not taken in yet, and the device counter of update calls."""

    def __init__(self, model, optimizer, enabled: bool, bf16: bool):
        self.model, self.optimizer, self.enabled, self.bf16 = model, optimizer, enabled, bf16
        self.step_dev = None       # ops.DeviceStepState
        self.draws, self.deltas, self.unsettled = 0, [], 0
        self.calls_seen = 0        # model._bf16_update_calls when the device counter last agreed with it (resync)
        self._hooks = []
        if enabled:
            settle = weakref.WeakMethod(self.settle)        # (the optimizer and the model must not keep this object alive)

            def _observed(*_args, _m=settle):
                f = _m()
                if f is not None:
                    f()
            # the observation points of the host mirrors: state_dict(), load_state_dict(), an eager optimizer step; the model calls the
            # same function in front of an eager bf16 key draw, which comes before the optimizer's own pre-hooks (a global hook)
            self._hooks = [optimizer.register_state_dict_pre_hook(_observed), optimizer.register_load_state_dict_pre_hook(_observed),
                           optimizer.register_step_pre_hook(_observed)]
            model._step_state_settle = _observed

    def __del__(self):
        try:
            self.settle()
            for h in self._hooks:
                h.remove()
        except Exception:                                   # noqa: BLE001 - interpreter shutdown
            pass

    def settle(self) -> None:
        """Host mirrors <- the replays since the last call: model._bf16_update_calls and every optimizer.state[p]["step"] the captured step
        advances read as if those replays had been eager steps.  Pure host arithmetic (a replay advances them by known amounts): no wait,
        no per-replay work — called where someone can observe the counters (the hooks of __init__, _drop_graph, a re-capture)."""
        n, self.unsettled = self.unsettled, 0
        if not n:
            return
        if self.draws:
            self.model._bf16_update_calls += self.draws * n
            self.calls_seen = self.model._bf16_update_calls
        state = self.optimizer.state
        for p, d in self.deltas:
            st = state.get(p)
            if st is not None and "step" in st:
                st["step"] = st["step"] + d * n

    def resync(self) -> None:
        """In front of a replay: EAGER bf16 update calls since the device counter was last written (a step taken outside this object) moved
        the host counter on; the device counter follows, written in stream order.  One comparison per replay otherwise."""
        sd = self.step_dev
        if sd is not None and self.model._bf16_update_calls != self.calls_seen:
            self.settle()           # (the eager draw settled already: nothing is pending; kept for a counter someone set by hand)
            self.calls_seen = self.model._bf16_update_calls
            sd.calls.fill_(self.calls_seen)

    @contextlib.contextmanager
    def capturing(self, dev, cap: Capture):
        """Around a capture, which starts from settled host counters: (calls, key) on the device, registered for its duration only.
        Afterwards: what one replay advances.  The capture RECORDED a step and ran none, yet its Python side advanced the optimizer's
        step counts: they are put back, so that every replay — the one that executes this step included — counts the same way."""
        self.settle()
        self.step_dev, self.draws, self.deltas = None, 0, []
        if not self.enabled:
            yield
            return
        state = self.optimizer.state
        before = {id(p): (st["step"].clone() if isinstance(st["step"], torch.Tensor) else st["step"]) for p, st in state.items() if "step" in st}
        if self.bf16:
            sd = self.step_dev = ops.DeviceStepState(self.model._bf16_update_calls, dev)
            self.calls_seen = self.model._bf16_update_calls
            ops._graph_step_state[id(self.model)] = sd
        try:
            yield
        finally:
            ops._graph_step_state.pop(id(self.model), None)
        for p, st in state.items():
            if "step" not in st:
                continue
            was = before.get(id(p), 0)
            d = st["step"] - was
            if float(d) != 0.0:
                st["step"] = was
                self.deltas.append((p, d))
        if self.bf16:
            if sd.draws < 1 or sd.draws != sd.passes:
                cap.reset()
                self.step_dev, self.deltas = None, []
                raise RuntimeError("dlrm_amd.graph: the captured step drew %d bf16 rounding keys for %d parked backward passes (one per pass "
                                   "is what a replay can follow); use the eager step" % (sd.draws, sd.passes))
            self.draws = sd.draws


def _held_by(owner: str, name: str):
    """an attribute of the step object that lives in one of its owners (the tests and tools read and set these names on the step)"""
    return property(lambda self: getattr(getattr(self, owner), name), lambda self, v: setattr(getattr(self, owner), name, v))


class GraphedTrainStep:
    """step = GraphedTrainStep(model, optimizer);  loss = step(X, lS_o, lS_i, T)   (loss: static 0-dim device tensor)

    The first `warmup` calls are ordinary eager steps (kernel attributes, workspaces and allocator pools settle); the
    next call captures the step and every call from then on copies its inputs into the static buffers and replays.
    `self.out` holds the predictions of the last step (static buffer)."""

    def __init__(self, model, optimizer, warmup: int = 2, device_step_state: bool = False):
        if ext_dist.is_distributed():       # (a forced one-rank group routes through distributed_forward as well: its RCCL calls must not be captured)
            raise RuntimeError("dlrm_amd.graph: the whole-step HIP graph is single-process only "
                               "(RCCL all-to-all / DDP all-reduce are not captured)")
        if getattr(model, "quantize_emb", False):
            sys.exit("ERROR: GraphedTrainStep captures a training step; a model with quantized embedding tables is inference only")
        if getattr(model, "quantize_mlp_bits", 32) != 32:
            sys.exit("ERROR: GraphedTrainStep captures a training step; a model with quantized MLP towers is inference only")
        if getattr(model, "_has_qr", None) is not None and model._has_qr(getattr(model, "emb_l", None)):
            sys.exit("ERROR: GraphedTrainStep is not built for QR embedding tables (their backward allocates the split index arrays per step)")
        if getattr(model, "_has_md", None) is not None and model._has_md(getattr(model, "emb_l", None)):
            sys.exit("ERROR: GraphedTrainStep is not built for mixed-dimension embedding tables (their backward builds the per-width bag lists per step)")
        # device_step_state (module docstring, "step state"): the per-step state of bf16 tables and of FusedAdagrad lives on the device / is
        # mirrored on the host, which lifts the next two refusals — but not for a stock torch.optim.Adagrad, whose dense step is torch's
        self.device_step_state = bool(device_step_state)
        self._bf16 = getattr(model, "emb_bf16", None) is not None
        if self._bf16 and not self.device_step_state:
            sys.exit("ERROR: GraphedTrainStep is not built for bfloat16 embedding tables (the per-step rounding seed would be baked into the capture)")
        if (type(optimizer).__name__ == "FusedAdagrad" and not self.device_step_state) or \
                (getattr(model, "fused_adagrad", False) and type(optimizer) is torch.optim.Adagrad):
            sys.exit("ERROR: GraphedTrainStep is not built for the fused exact Adagrad update (FusedAdagrad, or torch.optim.Adagrad with "
                     "model.fused_adagrad); use the eager step")
        self.model, self.optimizer = model, optimizer
        for g in optimizer.param_groups:
            # a decaying step size (RWSAdagrad: clr = lr / (1 + (step - 1) * lr_decay)) is computed on the host at capture time
            # and baked into kernel arguments: a replay would silently reuse a stale clr
            if float(g.get("lr_decay", 0.0) or 0.0) != 0.0:
                raise RuntimeError("dlrm_amd.graph: lr_decay != 0 changes the step size every step; a captured graph cannot "
                                   "follow it (use the eager step)")
        # Sort-based updates (DLRM_UPD_SORTED, the fused row-wise Adagrad): rocPRIM's onesweep radix sort ends in a memory-aperture
        # violation when REPLAYED from a HIP graph on ROCm 7.2 (tools/probes/graph_sorted_probe.py; the "TB-shape graph fault" of
        # profiles/r02/graph_probe.md).  Since round 3 of the build the library sorts table segments of up to 262144 lookups with its
        # own kernels (csrc/seg_sort.h: no memsets, no vendor code, replayable); whether THIS step's shapes are covered is only known
        # when the first batch arrives — decided in _settle_sort_mode().
        self._sort_checked = False
        self._one = None
        # the captured step is single-stream: a replayed graph has no launch gaps to hide, and the side-stream overlap
        # of the eager path (DLRM_Net.overlap_streams) would put cross-stream joins into the capture
        model.overlap_streams = False
        # ... and takes the whole sparse update at its optimizer step (the update-in-backward schedule of ABI 17 allocates its sorted
        # workspace per backward pass and binds to the optimizer's first EAGER step: not part of a captured step)
        model.update_in_backward = False
        self.warmup = max(int(warmup), 1)
        self.cap = Capture()        # stream, graph, raw handle, pinned scratch, out (the predictions of the last step)
        self.flight = InFlight()
        self.static = None
        self.plan: Optional[StagePlan] = None
        self.loss: Optional[torch.Tensor] = None
        self.lrs = DeviceLearningRates(optimizer)
        self.state = StepStateMirrors(model, optimizer, self.device_step_state, self._bf16)
        self.captures = 0
        self._eager_calls = 0
        self._keep = None
        # raw replay: wait + input copies + hipGraphLaunch in ONE C call (dlrm_graph_replay) instead of stream.synchronize(), a copy_ per
        # input and CUDAGraph.replay() from Python — the host path is what a launch-bound step waits for.  DLRM_GTS_RAW=0: the torch calls.
        self.raw = _os.environ.get("DLRM_GTS_RAW", "1") == "1"

    graph, stream, out, _exec = (_held_by("cap", n) for n in ("graph", "stream", "out", "exec"))
    _lr_on_device, lr_writes = _held_by("lrs", "on_device"), _held_by("lrs", "writes")
    _draws, _step_deltas, _unsettled = (_held_by("state", n) for n in ("draws", "deltas", "unsettled"))

    def _settle(self) -> None:
        self.state.settle()

    def _settle_sort_mode(self, lS_o, lS_i) -> None:
        """First batch: keep the sort-based embedding update only if every table segment goes through the library's own segmented
        sorter (ops.sort_is_graph_safe); otherwise SGD falls back to the atomic update and the row-wise Adagrad is refused."""
        if self._sort_checked:
            return
        self._sort_checked = True
        model, optimizer = self.model, self.optimizer
        adagrad = any(type(optimizer).__name__ == n for n in ("RWSAdagrad", "FusedRWSAdagrad", "FusedAdagrad"))
        what = "the fused %s Adagrad update" % ("exact" if type(optimizer).__name__ == "FusedAdagrad" else "row-wise")
        if self._bf16:
            # the bf16 update is sort-based whatever the optimizer and has no atomic form to fall back to: the Adagrad rule
            adagrad, what = True, "the bfloat16 table update"
        if not adagrad and getattr(model, "emb_update_mode", None) != ops.UPD_SORTED:
            return
        safe, lookups, why = False, 0, None
        try:
            bags = ops.BagBatch(lS_o, lS_i, None)
            safe = ops.sort_is_graph_safe([e.weight for e in model.emb_l], bags)
            lookups = int(sum(bags.nnz))
            # (decided once: every later batch has these segment sizes — _copy_struct refuses any other input shape)
        except Exception as e:                               # noqa: BLE001 - models without plain emb_l tables: be conservative
            safe, why = False, "%s: %s" % (type(e).__name__, e)
        # DLRM_GRAPH_SORTED: "1" keep the sorted update whenever it is replayable, "0" never, default "auto": keep it for batches of
        # >= 2^19 lookups (Criteo-Terabyte: 1.7 M) and take the atomic update for launch-bound batches, where the sort's nine small
        # launches cost more than its rows save (Criteo-Kaggle shapes, 53 k lookups: 0.83 ms sorted vs atomic, profiles/round3)
        pref = _os.environ.get("DLRM_GRAPH_SORTED", "auto")
        if pref == "0" or (pref == "auto" and not adagrad and lookups < (1 << 19)):
            safe = False
        if safe:
            return
        if adagrad:
            raise RuntimeError("dlrm_amd.graph: " + what + " of this batch cannot be replayed from a HIP graph: " +
                               ("the sorter check itself failed (%s)" % why if why else
                                "a table segment needs the general (rocPRIM) sorter, which cannot be replayed on this ROCm "
                                "(tools/probes/graph_sorted_probe.py)") + "; use the eager step")
        model.emb_update_mode = ops.UPD_ATOMIC               # LDS pre-reduction for tiny tables + hardware fp32 atomics

    def _prove_one_lookup_per_bag(self, lS_o, lS_i) -> None:
        """The fused lookup + interaction kernels are only valid for offsets == arange(B).  Eager steps prove that per offsets tensor
        (ops.offsets_are_iota, dlrm_amd/iota.py); inside a capture nothing can synchronise and the static offsets buffer is rewritten before every
        replay, so the proof is made HERE, on the caller's tensors, before they are copied.  A batch that fails it turns the fused
        path off for this model and drops the captured graph (the next call re-captures with the two kernels)."""
        model = self.model
        if not getattr(model, "fuse_emb_interact", False):
            return
        # (a model that cannot take the fused path anyway — Criteo-Kaggle's D = 16, a cat interaction, pooling weights — needs no proof: a
        # per-replay host wait doubled that launch-bound step when every replay brought a new offsets tensor)
        ask = getattr(model, "fused_route_now", None)
        if ask is not None:
            route = ask()
            if route is None or not route.none_fused:       # (undecided offsets inside the capture take the two-kernel form anyway)
                return
        n_i = lS_i.size(-1) if isinstance(lS_i, torch.Tensor) else None
        n_o = lS_o.size(-1) if isinstance(lS_o, torch.Tensor) else None
        if isinstance(lS_i, torch.Tensor) != isinstance(lS_o, torch.Tensor) or (n_i is not None and n_i != n_o):
            return                              # not the one-lookup shape: sequential_forward will not take the fused path
        if n_i is None and any(i.numel() != o.numel() for i, o in zip(lS_i, lS_o)):
            return
        if ops.offsets_are_iota(lS_o) is False:
            model.fuse_emb_interact = False
            self._drop_graph(lS_o)

    def _drop_graph(self, like) -> None:
        """forget the captured step (the next call re-captures): the replay in flight is waited for first, and the raw handle goes with
        the graph (Capture.reset)"""
        if self.cap.graph is None:
            return
        self.state.settle()
        dev = like.device if isinstance(like, torch.Tensor) else like[0].device
        torch.cuda.current_stream(dev).synchronize()
        self.flight.pending = False
        self.cap.reset()

    # one eager training step on the static buffers (the reference loop body)
    def _eager(self):
        X, lS_o, lS_i, T = self.static
        Z = self.model(X, lS_o, lS_i)
        E = self.model.loss_fn(Z, T)
        # E.backward() would run the parameters' AccumulateGrad nodes; those are created once and live as long as ANY
        # autograd graph references them (a loss tensor the caller kept from an earlier eager step is enough), on the
        # stream of that time — which breaks stream capture.  torch.autograd.grad returns the gradients without
        # AccumulateGrad; the embedding tables are listed so that their Function's backward (the fused-update stash)
        # runs, and come back as None exactly like after backward().
        params = [p for g in self.optimizer.param_groups for p in g["params"] if p.requires_grad]
        if self._one is None or self._one.device != E.device:
            self._one = torch.ones((), dtype=E.dtype, device=E.device)      # the seed of backward: without it autograd launches an ATen fill per step
        grads = torch.autograd.grad(E, params, grad_outputs=self._one, allow_unused=True)
        for p, g in zip(params, grads):
            p.grad = g
        self.optimizer.step()
        return Z, E

    def _capture(self, dev) -> None:
        self.cap.reset()             # (before the owners replace device state the previous graph reads)
        with self.lrs.capturing(dev), self.state.capturing(dev, self.cap):
            Z, E = self.cap.record(dev, self._eager, raw=self.raw)
        self.cap.out, self.loss = Z.detach(), E.detach()
        self.captures += 1

    def __call__(self, X, lS_o, lS_i, T):
        cap, flight = self.cap, self.flight
        request = (X, lS_o, lS_i, T)
        dev = X.device if self.static is None else self.static[0].device
        # the steady state: the request checked, then ONE call that waits for the previous replay, copies and launches (graph_core.replay)
        raw = False
        if cap.exec is not None and self.lrs.valid() and not _TRACE:    # (a raw handle: captured, after the warm-up calls)
            self._prove_one_lookup_per_bag(lS_o, lS_i)
            if cap.exec is not None:                        # (the proof may have dropped the graph)
                for s_, r in zip(self.static, request):
                    _check_struct(s_, r)
                raw = self.plan.takes(request)              # (host tensors, strided views: torch's copy_ handles them)
        if not raw:
            if _TRACE:
                print("[gts] call eager=%d captures=%d replay_in_flight=%s" % (self._eager_calls, self.captures, flight.pending),
                      flush=True)
            flight.wait(torch.cuda.current_stream(dev))     # before the static inputs are touched again (graph_core.InFlight)
            self._prove_one_lookup_per_bag(lS_o, lS_i)
            if self.static is None:
                self._settle_sort_mode(lS_o, lS_i)
                self.static = (X.clone(), _clone_struct(lS_o), _clone_struct(lS_i), T.clone())
                self.plan = StagePlan(self.static, request)
            else:
                for s_, r in zip(self.static, request):
                    _copy_struct(s_, r)
            if self._eager_calls < self.warmup:
                # the first calls are ordinary eager steps, issued on the stream the capture will use
                Z, E = cap.run(dev, self._eager)
                self._eager_calls += 1
                cap.out, self.loss = Z.detach(), E.detach()
                return self.loss
            if cap.graph is None or not self.lrs.valid():
                self._capture(dev)       # capture only records; the replay below executes this step
        scalars = self.lrs.changed()
        self.state.resync()
        replay(cap, flight, torch.cuda.current_stream(dev), self.plan, request, scalars=scalars, staged=not raw)
        self.state.unsettled += 1                           # (host mirrors of the step state: taken in lazily, settle)
        self._keep = request                                # the sources stay alive until the next call (their copies are asynchronous)
        return self.loss
