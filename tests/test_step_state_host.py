"""Step state of the whole-step graph (GraphedTrainStep(device_step_state=True)), the part that needs no GPU:

  * `key_sequence`: a restatement of the Philox key sequence dlrm_philox_key_next produces on the device (include/dlrm_hip.h, "STEP STATE ON
    THE DEVICE") in explicit wrap-around uint64 arithmetic, pinned against dlrm_net._mix_seed; tests/test_gpu_step_state.py imports it;
  * the constructor: bf16 tables and FusedAdagrad are accepted under the keyword, everything else it still refuses is refused in the same words;
  * the host mirrors: replays counted by the step are taken into model._bf16_update_calls and optimizer.state[p]["step"] at the observation
    points (state_dict, load_state_dict, an eager step, _settle itself), once.
"""
import copy

import numpy as np
import pytest
import torch

SEEDS = (0, 12345, 2 ** 63 + 0x1234567)          # (one >= 2^63: the products wrap and the key does not fit a signed word)


def key_sequence(seed0, first_call, count):
    """[key of update call first_call, ..., first_call + count - 1]: z = seed0 * 0x9E3779B97F4A7C15 + call * 0xBF58476D1CE4E5B9 (mod 2^64),
    key = z ^ (z >> 31) — numpy uint64 scalars wrap as the device's 64-bit registers do"""
    keys = []
    with np.errstate(over="ignore"):
        for n in range(first_call, first_call + count):
            z = np.uint64(seed0 & (2 ** 64 - 1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(n) * np.uint64(0xBF58476D1CE4E5B9)
            z ^= z >> np.uint64(31)
            keys.append(int(z))
    return keys


def as_u64(t):
    """int64 tensor (the device buffers hold the 64 bits of an unsigned word) -> python ints in [0, 2^64)"""
    return [int(v) & (2 ** 64 - 1) for v in t.detach().cpu().reshape(-1).tolist()]


def tiny_model(**kw):
    import dlrm_amd
    np.random.seed(11)
    torch.manual_seed(11)
    return dlrm_amd.DLRM_Net(8, np.asarray([300, 7, 3]), np.asarray([13, 8]), np.asarray([14, 1]), "dot", sigmoid_top=0, **kw)


@pytest.mark.parametrize("seed", SEEDS)
def test_key_sequence_restates_mix_seed(seed):
    from dlrm_amd.dlrm_net import _mix_seed
    assert key_sequence(seed, 0, 6) == [_mix_seed(seed, n) for n in range(6)]
    assert key_sequence(seed, 3, 3) == [_mix_seed(seed, n, 0) for n in (3, 4, 5)]
    assert len(set(key_sequence(seed, 0, 6))) == 6


# ------------------------------------------------------------------------------------------------ constructor
def test_bf16_tables_are_accepted_under_the_keyword():
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedRWSAdagrad, FusedSGD
    for make in (lambda p: torch.optim.SGD(p, lr=0.1), lambda p: FusedSGD(p, lr=0.1), lambda p: FusedRWSAdagrad(p, lr=0.1)):
        model = tiny_model()
        model.embedding_bfloat16()
        step = GraphedTrainStep(model, make(model.parameters()), device_step_state=True)
        assert step.device_step_state is True and step.captures == 0
        assert model.overlap_streams is False and model.update_in_backward is False
    # without it, the refusal of before
    model = tiny_model()
    model.embedding_bfloat16()
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for bfloat16 embedding tables"):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1), device_step_state=False)


def test_fused_adagrad_is_accepted_under_the_keyword_and_reads_lr_from_the_device():
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedAdagrad
    model = tiny_model()
    step = GraphedTrainStep(model, FusedAdagrad(model.parameters(), lr=0.1), device_step_state=True)
    assert step._lr_on_device is True
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for the fused exact Adagrad update"):
        GraphedTrainStep(model, FusedAdagrad(model.parameters(), lr=0.1))


def test_what_stays_refused_under_the_keyword():
    import dlrm_amd
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedAdagrad, FusedRWSAdagrad

    def sgd(m):
        return torch.optim.SGD(m.parameters(), lr=0.1)
    qr = tiny_model(qr_flag=True, qr_collisions=4, qr_threshold=100)
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for QR embedding tables"):
        GraphedTrainStep(qr, sgd(qr), device_step_state=True)
    md = dlrm_amd.DLRM_Net([8, 4, 8], np.asarray([300, 250, 3]), np.asarray([13, 8]), np.asarray([14, 1]), "dot", md_flag=True, md_threshold=200)
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for mixed-dimension embedding tables"):
        GraphedTrainStep(md, sgd(md), device_step_state=True)
    # quantised tables and towers: the state after quantize_embedding / quantize_mlp, set by hand (packing needs the GPU)
    q = tiny_model()
    opt = sgd(q)
    q.quantize_emb = True
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep captures a training step; a model with quantized embedding tables"):
        GraphedTrainStep(q, opt, device_step_state=True)
    q.quantize_emb, q.quantize_mlp_bits = False, 8
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep captures a training step; a model with quantized MLP towers"):
        GraphedTrainStep(q, opt, device_step_state=True)
    # a stock torch.optim.Adagrad with model.fused_adagrad: its dense step is torch's
    m = tiny_model()
    m.fused_adagrad = True
    with pytest.raises(SystemExit, match="ERROR: GraphedTrainStep is not built for the fused exact Adagrad update"):
        GraphedTrainStep(m, torch.optim.Adagrad(m.parameters(), lr=0.1), device_step_state=True)
    # a decaying step size
    for cls in (FusedAdagrad, FusedRWSAdagrad):
        m = tiny_model()
        with pytest.raises(RuntimeError, match="lr_decay != 0 changes the step size every step"):
            GraphedTrainStep(m, cls(m.parameters(), lr=0.1, lr_decay=0.01), device_step_state=True)
    q.quantize_mlp_bits = 32


# ------------------------------------------------------------------------------------------------ host mirrors
def _step_with_pending_replays(replays):
    """a step object in the state three replays of a captured bf16 + FusedRWSAdagrad step leave behind, set by hand (capturing needs the GPU):
    one key drawn and every parameter's step count advanced by one per replay"""
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedRWSAdagrad
    model = tiny_model()
    model.embedding_bfloat16()
    opt = FusedRWSAdagrad(model.parameters(), lr=0.1)
    step = GraphedTrainStep(model, opt, device_step_state=True)
    params = [p for g in opt.param_groups for p in g["params"]]
    for p in params:
        opt.state[p]["step"] = 3
    model._bf16_update_calls = 3
    step._draws, step._step_deltas, step._unsettled = 1, [(p, 1) for p in params], replays
    return model, opt, step, params


def test_state_dict_sees_the_replays_as_eager_steps_and_only_once():
    model, opt, step, params = _step_with_pending_replays(4)
    sd = opt.state_dict()
    assert all(st["step"] == 7 for st in sd["state"].values()) and len(sd["state"]) == len(params)
    assert model._bf16_update_calls == 7 and step._unsettled == 0
    assert all(st["step"] == 7 for st in opt.state_dict()["state"].values()) and model._bf16_update_calls == 7     # settled once


def test_load_state_dict_settles_first_so_that_the_loaded_counts_stand():
    model, opt, step, params = _step_with_pending_replays(4)
    saved = copy.deepcopy(opt.state_dict())      # (settles: 7; state_dict() hands out the live per-parameter dicts)
    step._unsettled = 2
    opt.load_state_dict(saved)
    assert all(opt.state[p]["step"] == 7 for p in params) and step._unsettled == 0
    assert model._bf16_update_calls == 9         # the model's counter is not the optimizer's to load
    step._unsettled = 1                          # the mirrors follow the state objects load_state_dict put in place
    step._settle()
    assert all(opt.state[p]["step"] == 8 for p in params) and model._bf16_update_calls == 10


def test_an_eager_key_draw_and_an_eager_optimizer_step_settle_first():
    from dlrm_amd.dlrm_net import _mix_seed
    model, opt, step, params = _step_with_pending_replays(4)
    assert model._step_state_settle is not None
    model._step_state_settle()                   # what _run_update calls in front of an eager draw
    assert model._bf16_update_calls == 7
    assert model._bf16_next_seed() == _mix_seed(model.emb_bf16[1], 7) and model._bf16_update_calls == 8
    step._unsettled = 2
    opt.step()                                   # no gradients: the step itself advances nothing; its pre-hook settles
    assert all(opt.state[p]["step"] == 9 for p in params) and model._bf16_update_calls == 10


def test_without_the_keyword_nothing_is_mirrored():
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedRWSAdagrad
    model = tiny_model()
    opt = FusedRWSAdagrad(model.parameters(), lr=0.1)
    step = GraphedTrainStep(model, opt)
    step._unsettled = 5
    assert all(st["step"] == 0 for st in opt.state_dict()["state"].values())
    assert model._step_state_settle is None


def test_a_discarded_step_object_leaves_no_hook_behind_that_keeps_it_alive():
    import gc
    import weakref
    model, opt, step, params = _step_with_pending_replays(2)
    ref = weakref.ref(step)
    del step
    gc.collect()
    assert ref() is None
    assert model._bf16_update_calls == 5         # settled on the way out
    opt.state_dict()                             # its hooks left with it


def test_a_param_group_added_after_the_capture_means_recapture_and_no_pointer_array():
    """The device learning rates are one scalar per param group OF THE CAPTURE.  The state a capture leaves behind, set by hand: a changed
    lr hands out the pointers and values of the replay's write; once a group is appended, the owner reports "re-capture" and hands out
    nothing — a write of len(param_groups) scalars would run past the captured buffer."""
    from dlrm_amd.graph import GraphedTrainStep
    from dlrm_amd.optim import FusedSGD
    model = tiny_model()
    opt = FusedSGD(model.parameters(), lr=0.1)
    step = GraphedTrainStep(model, opt)
    lrs = step.lrs
    assert step._lr_on_device is True and not lrs.valid()                # nothing captured yet
    lrs.dev, lrs.values = torch.zeros(len(opt.param_groups)), lrs.current()
    assert lrs.valid() and lrs.changed() is None and step.lr_writes == 0
    opt.param_groups[0]["lr"] = 0.25
    n, dst, values = lrs.changed()
    assert (n, dst[0], values[0]) == (1, lrs.dev.data_ptr(), 0.25) and step.lr_writes == 1 and lrs.valid()
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})
    assert not lrs.valid() and lrs.changed() is None
    opt.param_groups[0]["lr"] = 0.5                                      # ... whatever else changed meanwhile
    assert not lrs.valid() and lrs.changed() is None and step.lr_writes == 1 and lrs.values == [0.25]


def test_seed_argument_of_the_bf16_updates_is_an_int_or_a_one_element_int64_gpu_tensor():
    from dlrm_amd import ops
    assert ops._seed_args(2 ** 64 + 5) == (False, 5) and ops._seed_args(-1) == (False, 2 ** 64 - 1)
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="a device-side bf16 rounding seed must be a 1-element int64 GPU tensor"):
            ops._seed_args(bad)
    assert ops.device_step_state(object()) is None and ops._graph_step_state == {}
