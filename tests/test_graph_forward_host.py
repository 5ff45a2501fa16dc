"""GraphedForward (dlrm_amd/graph_forward.py), the part that needs no GPU: the bucket choice, the fixed-structure test on offsets, the
LRU of exact shapes, the segment lists of the staging call, the staleness fingerprint and the constructor's refusals."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graphed_forward_is_exported_from_graph():
    import dlrm_amd.graph as G
    from dlrm_amd.graph_forward import GraphedForward
    assert G.GraphedForward is GraphedForward


def test_pick_bucket_smallest_that_fits():
    from dlrm_amd.graph_forward import pick_bucket
    sizes = (256, 64, 2048)                     # (any order)
    assert [pick_bucket(n, sizes) for n in (1, 63, 64, 65, 256, 257, 2048)] == [64, 64, 64, 256, 256, 2048, 2048]
    assert pick_bucket(2049, sizes) is None     # above the largest: an exact-shape graph
    assert pick_bucket(5, None) is None and pick_bucket(5, ()) is None


def test_fixed_bag_lengths_on_lists_and_stacked():
    from dlrm_amd.graph_forward import fixed_bag_lengths
    n = 5
    one = [torch.arange(n) for _ in range(3)]
    ids = [torch.zeros(n, dtype=torch.int64) for _ in range(3)]
    assert fixed_bag_lengths(one, ids, n) == (1, 1, 1)
    # per-table fixed lengths: offsets == P * arange
    offs = [torch.arange(n), torch.arange(n) * 2, torch.arange(n) * 3]
    ids = [torch.zeros(n * p, dtype=torch.int64) for p in (1, 2, 3)]
    assert fixed_bag_lengths(offs, ids, n) == (1, 2, 3)
    # the right count of lookups with the wrong starts: an empty bag next to a two-lookup bag
    ragged = [torch.tensor([0, 0, 2, 3, 4]), torch.arange(n), torch.arange(n)]
    assert fixed_bag_lengths(ragged, [torch.zeros(n, dtype=torch.int64)] * 3, n) is None
    # a lookup count that is no multiple of n, fewer lookups than bags, another number of bags
    assert fixed_bag_lengths(one, [torch.zeros(n + 1, dtype=torch.int64)] * 3, n) is None
    assert fixed_bag_lengths(one, [torch.zeros(n - 1, dtype=torch.int64)] * 3, n) is None
    assert fixed_bag_lengths([torch.arange(n + 1)] * 3, [torch.zeros(n + 1, dtype=torch.int64)] * 3, n) is None
    # stacked [T, n]
    so = torch.arange(n).repeat(3, 1) * 2
    assert fixed_bag_lengths(so, torch.zeros((3, 2 * n), dtype=torch.int64), n) == (2, 2, 2)
    so2 = so.clone()
    so2[1, 2] += 1
    assert fixed_bag_lengths(so2, torch.zeros((3, 2 * n), dtype=torch.int64), n) is None
    # n == 1: the one bag starts at 0 whatever its length
    assert fixed_bag_lengths([torch.zeros(1, dtype=torch.int64)], [torch.zeros(4, dtype=torch.int64)], 1) == (4,)
    with pytest.raises(RuntimeError, match="must both be lists"):
        fixed_bag_lengths(one, torch.zeros((3, n), dtype=torch.int64), n)


def test_fixed_bag_lengths_verdict_follows_in_place_writes():
    from dlrm_amd.graph_forward import fixed_bag_lengths
    o = torch.arange(4) * 2
    ids = [torch.zeros(8, dtype=torch.int64)]
    assert fixed_bag_lengths([o], ids, 4) == (2,)
    o[1] = 3                                    # (a versioned write: the cached verdict is void)
    assert fixed_bag_lengths([o], ids, 4) is None


def test_lru_drops_least_recently_used():
    from dlrm_amd.graph_forward import LRU
    lru = LRU(2)
    assert lru.put("a", 1) == [] and lru.put("b", 2) == []
    assert lru.get("a") == 1                    # "a" is now the most recent
    assert lru.put("c", 3) == [2]
    assert lru.get("b") is None and sorted(lru.keys()) == ["a", "c"] and len(lru) == 2
    assert lru.put("a", 10) == [] and lru.get("a") == 10
    assert lru.put("d", 4) == [3]
    lru.clear()
    assert len(lru) == 0


def _ptr(a, j):
    return int(a[j] or 0)


def test_stage_plan_list_inputs_with_shared_offsets():
    from dlrm_amd.graph_forward import StagePlan, alias_pattern
    T, n, B = 3, 5, 8
    shared = torch.arange(n)
    X, lS_o, lS_i = torch.zeros((n, 4)), [shared] * T, [torch.zeros(n, dtype=torch.int64) for _ in range(T)]
    assert alias_pattern(lS_o) == (0, 0, 0) and alias_pattern(lS_i) is None
    so = torch.zeros(B, dtype=torch.int64)
    statics = (torch.zeros((B, 4)), [so] * T, [torch.zeros(B, dtype=torch.int64) for _ in range(T)])
    plan = StagePlan(statics, (X, lS_o, lS_i))
    assert plan.n == 1 + 1 + T                  # X, ONE offsets tensor, T index tensors
    plan.patch((X, lS_o, lS_i))
    assert [_ptr(plan.dst, j) for j in range(plan.n)] == [statics[0].data_ptr(), so.data_ptr()] + [t.data_ptr() for t in statics[2]]
    assert [_ptr(plan.src, j) for j in range(plan.n)] == [X.data_ptr(), shared.data_ptr()] + [t.data_ptr() for t in lS_i]
    assert list(plan.nbytes)[:plan.n] == [n * 4 * 4, n * 8] + [n * 8] * T
    assert plan.launches(4) == 1 and plan.launches(5) == 0
    # a group that is not staged (a bucket's offsets)
    plan = StagePlan((statics[0], None, statics[2]), (X, lS_o, lS_i))
    assert plan.n == 1 + T
    # more than 64 segments: two launches
    many = [torch.zeros(2, dtype=torch.int64) for _ in range(70)]
    plan = StagePlan(([torch.zeros(2, dtype=torch.int64) for _ in range(70)],), (many,))
    assert plan.n == 70 and plan.launches(4) == 2


def test_stage_plan_stacked_inputs():
    from dlrm_amd.graph_forward import StagePlan
    T, n, B = 3, 5, 8
    X, so, si = torch.zeros((n, 4)), torch.arange(n).repeat(T, 1), torch.zeros((T, n), dtype=torch.int32)
    # exact shape: three whole tensors, the memcpy path
    statics = (torch.zeros((n, 4)), torch.zeros((T, n), dtype=torch.int64), torch.zeros((T, n), dtype=torch.int32))
    plan = StagePlan(statics, (X, so, si))
    plan.patch((X, so, si))
    assert plan.n == 3 and plan.launches(4) == 0
    assert list(plan.nbytes)[:3] == [n * 16, T * n * 8, T * n * 4]
    # a bucket: the T rows of the request go to the heads of the T rows of the wider static buffer
    wide = torch.zeros((T, B), dtype=torch.int32)
    plan = StagePlan((torch.zeros((B, 4)), None, wide), (X, so, si), by_rows=(2,))
    plan.patch((X, so, si))
    assert plan.n == 1 + T
    assert [_ptr(plan.dst, j) for j in range(1, 1 + T)] == [wide.data_ptr() + k * B * 4 for k in range(T)]
    assert [_ptr(plan.src, j) for j in range(1, 1 + T)] == [si.data_ptr() + k * n * 4 for k in range(T)]
    assert list(plan.nbytes)[:plan.n] == [n * 16] + [n * 4] * T
    # patching again with a shorter request changes sources and lengths only
    X2, si2 = torch.zeros((2, 4)), torch.zeros((T, 2), dtype=torch.int32)
    before = [_ptr(plan.dst, j) for j in range(plan.n)]
    plan.patch((X2, so[:, :2].contiguous(), si2))
    assert [_ptr(plan.dst, j) for j in range(plan.n)] == before
    assert list(plan.nbytes)[:plan.n] == [2 * 16] + [2 * 4] * T
    with pytest.raises(RuntimeError, match="does not fit"):
        StagePlan((torch.zeros((B, 4)), None, torch.zeros((T, 4), dtype=torch.int32)), (X, so, si), by_rows=(2,))
    with pytest.raises(RuntimeError, match="staged by rows"):
        StagePlan((torch.zeros((B, 4)), None, wide), (X, so, si))          # narrower than its static and not named in by_rows
    with pytest.raises(RuntimeError, match="input structure differs"):
        StagePlan((torch.zeros((B, 4)), None, [wide]), (X, so, si))


def test_stage_plan_of_a_bucket_does_not_depend_on_the_request_it_was_built_from():
    """the plan of a bucket is built once, from whichever request comes first: built from one that FILLS the bucket it still stages a
    narrower one row by row (T rows laid end to end are not the heads of the T rows of the static buffer)"""
    from dlrm_amd.graph_forward import StagePlan
    T, B, n = 3, 8, 5
    wide, Xs = torch.zeros((T, B), dtype=torch.int32), torch.zeros((B, 4))
    full = (torch.zeros((B, 4)), torch.arange(B).repeat(T, 1), torch.zeros((T, B), dtype=torch.int32))
    short = (torch.zeros((n, 4)), torch.arange(n).repeat(T, 1), torch.ones((T, n), dtype=torch.int32))
    plans = [StagePlan((Xs, None, wide), like, by_rows=(2,)) for like in (full, short)]
    assert plans[0].entries == plans[1].entries == [(0, None, None)] + [(2, None, k) for k in range(T)]
    for plan in plans:
        plan.patch(short)
        assert [_ptr(plan.dst, j) for j in range(plan.n)] == [Xs.data_ptr()] + [wide.data_ptr() + k * B * 4 for k in range(T)]
        assert [_ptr(plan.src, j) for j in range(plan.n)] == [short[0].data_ptr()] + [short[2].data_ptr() + k * n * 4 for k in range(T)]
        assert list(plan.nbytes)[:plan.n] == [n * 16] + [n * 4] * T
        plan.patch(full)
        assert list(plan.nbytes)[:plan.n] == [B * 16] + [B * 4] * T
    # the copies themselves, on the host: rows land in their own rows, the tails stay
    plan = plans[0]
    plan.patch(short)
    import ctypes
    wide.fill_(7)
    for j in range(1, plan.n):
        ctypes.memmove(_ptr(plan.dst, j), _ptr(plan.src, j), plan.nbytes[j])
    assert torch.equal(wide[:, :n], short[2]) and bool((wide[:, n:] == 7).all())
    # nothing longer than its destination is ever handed to the copy
    with pytest.raises(RuntimeError, match="larger than the static buffer"):
        plan.patch((torch.zeros((B + 1, 4)), None, torch.zeros((T, B), dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="larger than the static buffer"):
        plan.patch((torch.zeros((n, 4)), None, torch.zeros((T, B + 1), dtype=torch.int32)))


def test_vouch_offsets_is_a_public_hook_of_the_proof_cache():
    from dlrm_amd import iota
    o = torch.tensor([0, 0, 2])
    assert iota._iota_cached(o) is None
    iota.vouch_offsets(o, False)
    assert iota._iota_cached(o) is False
    iota.vouch_offsets(o, True)
    assert iota._iota_cached(o) is True
    o[1] = 1                                    # a versioned write voids it, as for a proof's own verdict
    assert iota._iota_cached(o) is None


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 2)
        self.b = torch.nn.Linear(2, 1)
        self.quantize_bits, self.quantize_mlp_bits, self.emb_bf16, self.quantize_emb = 32, 32, None, False

    def _table_kind(self):
        return "fp32"


def test_fingerprint_sees_scalars_and_moved_tensors_not_in_place_writes():
    from dlrm_amd.graph_forward import fingerprint, model_tensors
    m = _Stub()
    ts = model_tensors(m)
    assert [t.data_ptr() for t in ts] == [p.data_ptr() for p in m.parameters()]
    fp = fingerprint(m, ts)
    with torch.no_grad():
        m.a.weight.add_(1.0)                    # training between requests: in place, nothing to do
    assert fingerprint(m, ts) == fp
    m.quantize_mlp_bits = 16
    assert fingerprint(m, ts) != fp
    m.quantize_mlp_bits = 32
    m.emb_bf16 = "stochastic"
    assert fingerprint(m, ts) != fp
    m.emb_bf16 = None
    assert fingerprint(m, ts) == fp
    m.a.weight.data = m.a.weight.data.clone()   # the Parameter stays, its storage moved (what embedding_bfloat16 does to a table)
    assert fingerprint(m, ts) != fp
    m2 = _Stub()
    fp2 = fingerprint(m2, model_tensors(m2))
    m2.b.bias.data = m2.b.bias.data.clone()     # ... and the last one
    assert fingerprint(m2, model_tensors(m2)) != fp2
    # packed tables come first
    m3 = _Stub()
    m3.quantize_emb, m3.emb_l_q = True, [torch.zeros(4, dtype=torch.uint8)]
    assert model_tensors(m3)[0] is m3.emb_l_q[0]


def test_constructor_refuses_int8_towers_with_buckets():
    from dlrm_amd.graph import GraphedForward
    m = _Stub()
    m.quantize_mlp_bits = 8
    with pytest.raises(SystemExit, match="ERROR: .*int8 towers quantise per batch; padded buckets would change the result"):
        GraphedForward(m, batch_sizes=(8, 32))
    fwd = GraphedForward(m)                     # exact-shape graphs work
    assert fwd.batch_sizes is None and fwd.captures == 0 and fwd.replays == 0 and fwd.staged_launches == 0 and fwd.buckets_in_use == 0
    m.quantize_mlp_bits = 16                    # fp16 towers are row-independent
    assert GraphedForward(m, batch_sizes=(32, 8, 8)).batch_sizes == (8, 32)


def test_a_cpu_model_is_refused_at_the_first_call():
    from dlrm_amd.graph import GraphedForward
    fwd = GraphedForward(_Stub())
    with pytest.raises(RuntimeError, match="move the model to the GPU first"):
        fwd(torch.zeros((2, 3)), [torch.arange(2)], [torch.zeros(2, dtype=torch.int64)])
    assert fwd.captures == 0 and fwd.exact_shapes == 0


def test_constructor_refuses_distributed(monkeypatch):
    from dlrm_amd import ext_dist
    from dlrm_amd.graph import GraphedForward
    monkeypatch.setattr(ext_dist, "is_distributed", lambda: True)
    with pytest.raises(RuntimeError, match="whole-forward HIP graph is single-process only"):
        GraphedForward(_Stub())


def test_evaluate_inference_has_the_graphed_keyword_default_off():
    import inspect
    from dlrm_amd import evaluate
    p = inspect.signature(evaluate.inference).parameters["graphed"]
    assert p.default is False


def test_abi_symbols_declared_and_version_unchanged():
    """the two symbols are additive: declared in the header, bound in _lib.SIGNATURES, built from csrc/stage.hip, ABI version still 17"""
    from dlrm_amd import _lib
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    for name in ("dlrm_stage_inputs", "dlrm_forward_replay"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    assert _lib.EXPECTED_ABI == 17
    assert "stage.hip" in open(os.path.join(ROOT, "dlrm_amd", "csrc", "Makefile")).read()
    assert _lib.SIGNATURES["dlrm_stage_inputs"][1] == [C.c_int, _lib._pp, _lib._pp, _lib._pi64, C.c_void_p]
