"""Ragged buckets of GraphedForward (lookup_capacity=...), the part that needs no GPU: the routing order and the keys, the capacities, the
refusals, the shift arithmetic of graph_core.RaggedPlan against a pure-Python model of the staging, the exact-shape fallback, the two new
symbols, and the well-formedness of every oracle batch the GPU tests build (tests/ragged_cases.py)."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import ragged_cases as R
from ragged_cases import BATCH_SIZES, CAPACITY, EDGE_CASES, M_DEN, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(M_DEN, 1)
        self.quantize_bits, self.quantize_mlp_bits, self.emb_bf16, self.quantize_emb = 32, 32, None, False

    def _table_kind(self):
        return "fp32"


def _fwd(**kw):
    from dlrm_amd.graph import GraphedForward
    kw.setdefault("batch_sizes", BATCH_SIZES)
    kw.setdefault("lookup_capacity", CAPACITY)
    return GraphedForward(_Stub(), **kw)


def test_routing_fixed_length_then_ragged_then_exact():
    fwd = _fwd()
    # exactly two lookups in every bag: the fixed-length bucket, as without lookup_capacity
    fixed = R.make_request(5, 1, lens=[[2] * 5] * T)
    g = fwd._lookup(*fixed)
    assert g.key[0] == "bucket" and g.key[1] == 8 and g.key[6] == (2, 2, 2)
    # bags of their own lengths: the ragged bucket; its key holds the capacities and no nnz
    a, b = R.make_request(5, 2), R.make_request(7, 3)
    assert [i.numel() for i in a[2]] != [i.numel() for i in b[2]]
    ga, gb = fwd._lookup(*a), fwd._lookup(*b)
    assert ga is gb and ga.key == ("ragged", 8, False, M_DEN, torch.float32, torch.int64, (3, 3, 3), (None, None))
    assert ga.bucket == 8 and ga.n == 8 and ga.iota is None
    Xs, Os, Is = ga.static
    assert Xs.shape == (8, M_DEN) and int(Xs.abs().sum()) == 0
    assert all(o.shape == (8,) and bool((o == 24).all()) for o in Os) and all(i.shape == (24,) and int(i.abs().sum()) == 0 for i in Is)
    # the next bucket, another dtype, stacked inputs and a shared offsets tensor are other keys
    big = fwd._lookup(*R.make_request(9, 4))
    assert big.key[:2] == ("ragged", 32) and big.plan.caps == (96, 96, 96)
    assert fwd._lookup(*R.make_request(5, 5, idt=torch.int32)).key[5] == torch.int32
    X, offs, ids = R.make_request(5, 6, same_nnz=True)
    gs = fwd._lookup(X, torch.stack(offs), torch.stack(ids))
    assert gs.key[2] is True and gs.key[7] is None and gs.static[1].shape == (T, 8) and gs.static[2].shape == (T, 24) and gs.plan.stacked
    X, offs, ids = R.make_request(5, 7, lens=[[1, 0, 3, 2, 0]] * T)
    gsh = fwd._lookup(X, [offs[0]] * T, ids)
    assert gsh.key[7] == ((0, 0, 0), None) and gsh.static[1][0] is gsh.static[1][2] and (gsh.plan.n_ids, gsh.plan.n_off) == (T, 1)
    # above the largest bucket, or above the capacity: an exact-shape graph
    assert fwd._lookup(*R.make_request(33, 8)).key[0] == "exact"
    over = R.make_request(8, 9, lens=[[4, 3] * 4, [1] * 8, [0, 1] * 4])
    assert over[2][0].numel() == 28 and fwd._lookup(*over).key[0] == "exact"
    assert fwd.exact_shapes == 2 and len(fwd._buckets) == 6 and fwd.ragged_buckets_in_use == 0        # (nothing captured yet)


def test_without_lookup_capacity_nothing_changes():
    fwd = _fwd(lookup_capacity=None)
    assert fwd.lookup_capacity is None and fwd._lookup(*R.make_request(5, 2)).key[0] == "exact"
    assert fwd._lookup(*R.make_request(5, 1, lens=[[2] * 5] * T)).key[0] == "bucket"


def test_capacities_from_an_int_and_from_a_sequence():
    from dlrm_amd.graph_forward import lookup_capacities
    assert lookup_capacities(None) is None and lookup_capacities(3) == (3,) and lookup_capacities(3, 4) == (3, 3, 3, 3)
    assert lookup_capacities([1, 2, 3], 3) == (1, 2, 3) and lookup_capacities((5,), 1) == (5,)
    fwd = _fwd(lookup_capacity=(1, 2, 4))
    g = fwd._lookup(*R.make_request(6, 10, lens=[[1, 0, 2, 1, 0, 1], [3, 0, 0, 3, 3, 3], [4, 4, 0, 1, 5, 3]]))
    assert g.key[0] == "ragged" and g.key[6] == (1, 2, 4) and g.plan.caps == (8, 16, 32)
    assert [i.numel() for i in g.static[2]] == [8, 16, 32] and [int(o[0]) for o in g.static[1]] == [8, 16, 32]
    g32 = fwd._lookup(*R.make_request(20, 11, max_len=1))
    assert g32.plan.caps == (32, 64, 128)
    # stacked inputs have ONE width: unequal capacities leave them to the exact-shape graphs
    X, offs, ids = R.make_request(5, 12, same_nnz=True, max_len=1)
    assert fwd._lookup(X, torch.stack(offs), torch.stack(ids)).key[0] == "exact"
    # Lcap_k == bucket for every table and no fused route in the model: nothing to vouch for
    assert _fwd(lookup_capacity=1)._lookup(*R.make_request(6, 13, lens=[[0, 2, 1, 1, 1, 1]] * T)).iota is None


def test_refusals():
    from dlrm_amd.graph import GraphedForward
    from dlrm_amd.graph_forward import RaggedPlan, ragged_fits
    with pytest.raises(ValueError, match="needs batch_sizes"):
        GraphedForward(_Stub(), lookup_capacity=3)
    for bad in (0, -1, 2.5, "3", True, (), (3, 0, 3), [3, None, 3]):
        with pytest.raises(ValueError, match="lookup_capacity is an int >= 1"):
            _fwd(lookup_capacity=bad)
    with pytest.raises(ValueError, match="names 2 tables, the request has 3"):
        _fwd(lookup_capacity=(3, 3))._lookup(*R.make_request(5, 2))
    m = _Stub()
    m.quantize_mlp_bits = 8                     # int8 towers stay refused with buckets
    with pytest.raises(SystemExit, match="int8 towers quantise per batch"):
        GraphedForward(m, batch_sizes=BATCH_SIZES, lookup_capacity=3)
    # one offsets tensor for tables of unequal nnz: no ragged bucket (one static buffer has one shift), and the plan refuses it too
    X, offs, ids = R.make_request(5, 14, lens=[[1, 0, 3, 2, 0]] * T)
    ids[1] = ids[1][:4]
    shared = [offs[0]] * T
    assert ragged_fits([o.clone() for o in shared], ids, 5, (24,) * T) and not ragged_fits(shared, ids, 5, (24,) * T)
    fwd = _fwd()
    assert fwd._lookup(X, shared, ids).key[0] == "exact"
    so = torch.full((8,), 24)
    plan = RaggedPlan((torch.zeros((8, M_DEN)), [so] * T, [torch.zeros(24, dtype=torch.int64) for _ in range(T)]), (24,) * T, 8)
    with pytest.raises(RuntimeError, match="share one offsets tensor need the same number of lookups"):
        plan.patch((X, shared, ids))
    with pytest.raises(RuntimeError, match="share one offsets tensor need one lookup capacity"):
        RaggedPlan((torch.zeros((8, M_DEN)), [so] * T, [torch.zeros(c, dtype=torch.int64) for c in (24, 24, 16)]), (24, 24, 16), 8)
    # a request that does not fit is refused by patch(): rows, lookups, offsets count, dtype
    plan = RaggedPlan((torch.zeros((8, M_DEN)), [torch.full((8,), 24) for _ in range(T)], [torch.zeros(24, dtype=torch.int64) for _ in range(T)]),
                      (24,) * T, 8)
    X, offs, ids = R.make_request(5, 15)
    plan.patch((X, offs, ids))
    with pytest.raises(RuntimeError, match="dense input does not fit"):
        plan.patch((torch.zeros((9, M_DEN)), offs, ids))
    with pytest.raises(RuntimeError, match="does not fit its bucket"):
        plan.patch((X, offs, [torch.zeros(25, dtype=torch.int64)] + ids[1:]))
    with pytest.raises(RuntimeError, match="does not fit its bucket"):
        plan.patch((X, [offs[0][:4]] + offs[1:], ids))
    with pytest.raises(RuntimeError, match="does not fit its bucket"):
        plan.patch((X, offs, [ids[0].to(torch.int32)] + ids[1:]))
    with pytest.raises(RuntimeError, match="input structure differs"):
        plan.patch((X, torch.stack(offs), torch.zeros((T, 5), dtype=torch.int64)))


def _model_staging(plan, static, request):
    """the staging as the issue defines it, in plain Python on host tensors (what stage_ragged_kernel does with the plan's arguments)"""
    X, offs, ids = request
    Xs, Os, Is = static
    n, B = X.size(0), plan.bucket
    Xs[:n] = X
    for k in range(plan.T):
        cap, nnz = plan.caps[k], ids[k].numel()
        shift = cap - nnz
        Is[k][shift:] = ids[k]
        Os[k][:n] = shift + offs[k].clamp(0, nnz)
        Os[k][n:B] = cap


def _bags(offs, ids, bags, nnz):
    """bag b = ids[off[b] : off[b + 1]], the last one ends at nnz — as every lookup kernel reads them"""
    ends = offs.tolist()[1:] + [nnz]
    return [ids[s:e].tolist() for s, e in zip(offs.tolist()[:bags], ends)]


@pytest.mark.parametrize("idt", (torch.int64, torch.int32))
def test_shift_arithmetic_of_patch_against_a_model(idt):
    from dlrm_amd.graph_forward import RaggedPlan
    caps = (24, 24, 24)
    static = (torch.zeros((8, M_DEN)), [torch.full((8,), 24, dtype=idt) for _ in range(T)], [torch.zeros(24, dtype=idt) for _ in range(T)])
    plan = RaggedPlan(static, caps, 8)
    assert plan.elem == (8 if idt == torch.int64 else 4) and (plan.n_ids, plan.n_off) == (T, T)
    dst_before = [plan.ids_dst[j] for j in range(T)] + [plan.off_dst[j] for j in range(T)]
    assert dst_before == [t.data_ptr() for t in static[2]] + [t.data_ptr() for t in static[1]]
    reqs = [R.make_request(n, 20 + k, lens=lens, idt=idt) for k, (_, n, lens) in enumerate(EDGE_CASES)]
    for req in reqs + reqs[:2]:                 # (again after the others: stale heads and tails)
        X, offs, ids = req
        n = X.size(0)
        plan.patch(req)
        nnz = [i.numel() for i in ids]
        assert plan.nnz == nnz and plan.shift == [24 - z for z in nnz] and plan.rows == n and plan.x_bytes == n * M_DEN * 4
        assert [plan.ids_nnz[j] for j in range(T)] == nnz and [plan.off_nnz[j] for j in range(T)] == nnz
        assert [plan.ids_cap[j] for j in range(T)] == [24] * T and [plan.off_cap[j] for j in range(T)] == [24] * T
        assert [plan.ids_src[j] for j in range(T)] == [i.data_ptr() if i.numel() else None for i in ids]
        assert [plan.off_src[j] for j in range(T)] == [o.data_ptr() for o in offs] and plan.x_src == X.data_ptr()
        assert [plan.ids_dst[j] for j in range(T)] + [plan.off_dst[j] for j in range(T)] == dst_before
        assert plan.launches() == 1 and plan.args()[-3:] == (n, 8, plan.elem)
        _model_staging(plan, static, req)
        # the static buffers now hold the request's bags, id for id, and empty tail bags — with nnz = Lcap baked in
        for k in range(T):
            got = _bags(static[1][k], static[2][k], 8, 24)
            assert got[:n] == _bags(offs[k], ids[k], n, nnz[k]) and got[n:] == [[]] * (8 - n)
            assert int(static[1][k][0]) == plan.shift[k]
        assert torch.equal(static[0][:n], X)
    # more segments than one launch holds
    many = RaggedPlan((torch.zeros((2, 1)), [torch.full((2,), 4) for _ in range(40)], [torch.zeros(4, dtype=torch.int64) for _ in range(40)]),
                      (4,) * 40, 2)
    many.patch((torch.zeros((1, 1)), [torch.zeros(1, dtype=torch.int64) for _ in range(40)], [torch.zeros(2, dtype=torch.int64) for _ in range(40)]))
    assert many.launches() == 2


def test_stacked_plan_stages_by_rows():
    from dlrm_amd.graph_forward import RaggedPlan
    Os, Is = torch.full((T, 8), 24, dtype=torch.int32), torch.zeros((T, 24), dtype=torch.int32)
    plan = RaggedPlan((torch.zeros((8, M_DEN)), Os, Is), (24,) * T, 8)
    X, offs, ids = R.make_request(5, 30, same_nnz=True, idt=torch.int32)
    so, si = torch.stack(offs), torch.stack(ids)
    w = si.size(1)
    plan.patch((X, so, si))
    assert [plan.ids_dst[k] for k in range(T)] == [Is.data_ptr() + k * 24 * 4 for k in range(T)]
    assert [plan.off_dst[k] for k in range(T)] == [Os.data_ptr() + k * 8 * 4 for k in range(T)]
    assert [plan.ids_src[k] for k in range(T)] == [si.data_ptr() + k * w * 4 for k in range(T)]
    assert [plan.off_src[k] for k in range(T)] == [so.data_ptr() + k * 5 * 4 for k in range(T)]
    assert plan.shift == [24 - w] * T and plan.elem == 4
    with pytest.raises(RuntimeError, match="does not fit its bucket"):
        plan.patch((X, so, torch.zeros((T, 25), dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="one capacity for all tables"):
        RaggedPlan((torch.zeros((8, M_DEN)), Os, Is), (24, 24, 16), 8)


def test_every_oracle_batch_of_the_gpu_tests_is_well_formed():
    """the padded batches of tests/test_gpu_graph_ragged.py: offsets that start at 0, never decrease and end inside the ids; the requests of
    the capture-count cases stay within capacity, and none of them has a fixed lookup structure (that would be the other bucket kind)"""
    from dlrm_amd.graph_forward import fixed_bag_lengths, ragged_fits
    reqs = [(8, R.make_request(n, 100 + k, lens=lens)) for k, (_, n, lens) in enumerate(EDGE_CASES)]
    reqs += [(32, R.make_request(n, 120 + k)) for k, n in enumerate((9, 32, 20))]
    reqs += [(8, R.make_request(6, 210 + k)) for k in (1, 5)] + [(8, R.make_request(8, 600 + s)) for s in range(2)]
    reqs += [(8, R.make_request(n, 330 + k, same_nnz=True)) for k, n in enumerate((5, 8, 3, 7))]
    reqs += [(8, R.make_request(n, 330 + k)) for k, n in enumerate((5, 8, 3, 7))]
    reqs += [(n, R.make_request(n, 700 + k)) for k, n in enumerate((8, 8, 32, 8, 32, 8))]
    for bucket, req in reqs:
        X, offs, ids = req
        n = X.size(0)
        assert R.well_formed(offs, ids, n)
        Xp, op, ip = R.padded(bucket, *req)
        assert R.well_formed(op, ip, bucket) and Xp.shape == (bucket, M_DEN) and int(Xp[n:].abs().sum()) == 0
        assert ragged_fits(offs, ids, n, (bucket * CAPACITY,) * T) and fixed_bag_lengths(offs, ids, n) is None
    shapes = {(r[0].size(0),) + tuple(i.numel() for i in r[2]) for _, r in reqs[-6:]}
    assert len(shapes) == 6                     # (evaluate.inference's batches: every one a shape of its own)


def test_abi_symbols_declared_and_version_unchanged():
    from dlrm_amd import _lib, evaluate
    header = open(os.path.join(ROOT, "include", "dlrm_hip.h")).read()
    for name in ("dlrm_stage_ragged", "dlrm_forward_replay_ragged"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    assert _lib.EXPECTED_ABI == 17
    stage = _lib.SIGNATURES["dlrm_stage_ragged"][1]
    assert len(stage) == 17 and stage[-4:] == [C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    assert _lib.SIGNATURES["dlrm_forward_replay_ragged"][1] == stage[:-1] + [C.c_void_p, C.c_int, C.c_void_p]
    lib = _lib.load()
    assert lib.dlrm_hip_abi_version() == 17 and hasattr(lib, "dlrm_stage_ragged") and hasattr(lib, "dlrm_forward_replay_ragged")
    # refused on the host, before anything touches a device: n > bucket, and no graph to launch
    assert lib.dlrm_stage_ragged(None, None, 0, 0, None, None, None, None, 0, None, None, None, None, 9, 8, 8, None) == -1
    assert lib.dlrm_forward_replay_ragged(None, None, 0, 0, None, None, None, None, 0, None, None, None, None, 1, 8, 8, None, 0, None) == -1
    p = inspect.signature(evaluate.inference).parameters
    assert p["batch_sizes"].default is None and p["lookup_capacity"].default is None and p["graphed"].default is False
