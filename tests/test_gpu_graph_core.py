"""GraphedTrainStep on the shared capture-and-replay core (dlrm_amd/graph_core.py), against an eager twin, bit for bit:

  * every input form a replay stages — stacked [T, B] tensors (one segment each), lists that share one offsets tensor (one segment per
    distinct tensor), X as a strided view (torch's copy_ path, then torch's replay) — through the raw replay call and through torch's;
  * a param group added after the capture: the next call re-captures, nothing is written past the captured learning-rate scalars.

The tiny model of tests/test_step_state_host.py (tables of 300 / 7 / 3 rows, D = 8, towers 13-8 and 14-1), B = 64, deterministic update,
FusedSGD."""
import numpy as np
import pytest
import torch

import test_step_state_host as S

pytestmark = pytest.mark.gpu

ROWS = (300, 7, 3)
B = 64
NBATCH = 7
_batches = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    return torch.device("cuda:0")


def batches():
    """NBATCH batches, one lookup per bag, built once: (X, the offsets tensor the tables share, [T, B] indices, targets)"""
    if not _batches:
        rng = np.random.default_rng(404)
        off = torch.arange(B, dtype=torch.int64, device=dev())
        for s in range(NBATCH):
            X = torch.from_numpy(rng.uniform(0.0, 1.0, size=(B, 13)).astype(np.float32)).to(dev())
            idx = torch.from_numpy(np.stack([rng.integers(0, n, size=B, dtype=np.int64) for n in ROWS])).to(dev())
            Y = torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32)).to(dev())
            _batches[s] = (X, off, idx, Y)
    return _batches


def request(form, s):
    """-> (what the graphed step is called with, what the eager twin is called with)"""
    X, off, idx, Y = batches()[s]
    if form == "stacked":
        r = (X, off.unsqueeze(0).repeat(len(ROWS), 1), idx, Y)
        return r, r
    lists = ([off] * len(ROWS), [idx[k] for k in range(len(ROWS))])
    if form == "lists":
        return (X, *lists, Y), (X, *lists, Y)
    wide = torch.zeros((B, 26), dtype=X.dtype, device=X.device)
    wide[:, :13] = X
    assert not wide[:, :13].is_contiguous()
    return (wide[:, :13], *lists, Y), (X, *lists, Y)


def build():
    from dlrm_amd import ops
    from dlrm_amd.optim import FusedSGD
    model = S.tiny_model().to(dev())
    model.emb_update_mode = ops.UPD_DETERMINISTIC
    return model, FusedSGD(model.parameters(), lr=0.1)


def twins():
    from dlrm_amd.graph import GraphedTrainStep
    me, oe = build()
    mg, og = build()
    step = GraphedTrainStep(mg, og, warmup=2)
    me.overlap_streams, me.update_in_backward = mg.overlap_streams, mg.update_in_backward      # the schedule the constructor forced on mg
    return (me, oe), (mg, og), step


def eager_step(model, opt, X, lS_o, lS_i, Y):
    E = model.loss_fn(model(X, lS_o, lS_i), Y)
    opt.zero_grad()
    E.backward()
    opt.step()
    return float(E.detach())


def assert_same_parameters(eager, graphed):
    torch.cuda.synchronize()
    for (k, v), (kg, vg) in zip(eager[0].state_dict().items(), graphed[0].state_dict().items()):
        assert k == kg and torch.equal(v.view(torch.int32), vg.view(torch.int32)), k
    for ge, gg in zip(eager[1].param_groups, graphed[1].param_groups):
        for p, q in zip(ge["params"], gg["params"]):
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))


@pytest.mark.parametrize("raw", ["1", "0"])
@pytest.mark.parametrize("form", ["stacked", "lists", "strided-x"])
def test_six_graphed_steps_equal_eager_for_every_input_form(form, raw, monkeypatch):
    monkeypatch.setenv("DLRM_GTS_RAW", raw)
    eager, graphed, step = twins()
    le, lg = [], []
    for s in range(6):                                      # 2 warm-up calls, the capture, 3 replays more
        rg, re_ = request(form, s)
        lg.append(float(step(*rg)))
        le.append(eager_step(*eager, *re_))
    assert le == lg, (le, lg)
    assert_same_parameters(eager, graphed)
    assert step.captures == 1
    assert (step._exec is not None) == (raw == "1")
    assert step.plan.n == {"stacked": 4, "lists": 1 + 1 + len(ROWS) + 1, "strided-x": 1 + 1 + len(ROWS) + 1}[form]
    assert step.plan.takes(request(form, 0)[0]) == (form != "strided-x")


def test_a_param_group_added_after_the_capture_recaptures_and_equals_eager():
    eager, graphed, step = twins()
    le, lg = [], []

    def both(s):
        rg, re_ = request("lists", s)
        lg.append(float(step(*rg)))
        le.append(eager_step(*eager, *re_))
    for s in range(5):                                      # 2 warm-up calls, the capture and 3 replays in all
        both(s)
    assert step.captures == 1
    captured_scalars = step.lrs.dev.numel()
    for _, opt in (eager, graphed):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(5, device=dev()))], "lr": 0.05})
    both(5)
    assert step.captures == 2 and step.lrs.dev.numel() == captured_scalars + 1
    for s in (6, 0, 1):                                     # three steps more on the re-captured graph
        both(s)
    assert step.captures == 2
    assert le == lg, (le, lg)
    assert_same_parameters(eager, graphed)
